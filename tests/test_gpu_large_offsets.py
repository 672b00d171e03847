"""Every feature-side entry point at byte offsets past 2^31 and 2^32: source tables, shards, tiers, outputs.

The product's tables do not fit 32-bit offsets (papers100M: 56.9 GB of features).  Each test here allocates one array of
a little more than 4 GiB with torch.empty, fills it on the device with graphgen's aperiodic feature code (so the row a
truncated offset would land on has OTHER contents, test_feature_code.py) and calls the entry point with an index that
holds
  * the ~70 rows on either side of the 2^31-byte and of the 2^32-byte boundary (a row that straddles one included),
  * the rows a truncated offset would land on: the first ~70 rows of the table, and those just past 2^31 bytes,
  * a few hundred random rows,
unsorted, with repeats, and of a count that is no multiple of 64.  What a row must hold comes from the code's torch twin
applied to the ids (or from the feat_formats yardsticks applied to the stored bytes read back with plain torch indexing),
never from the kernel under test; outputs lie between canaries.  Every comparison is bit-exact.  No index is ever out of
range of its table, whatever a kernel does with it.

What these tests see that the suite did not: with PlainRows::row (extract.hip) cutting row * row_bytes to 32 bits, every
gather test on the former periodic feature pattern passed, both full-size ones included; the plain, long-row and
converting gathers here failed, and so did the full-size papers100M test on the aperiodic code.  (The other locators
compute their own offsets; that one-line change does not reach them.)"""
import numpy as np
import pytest

import feat_formats as ff
from feat_formats import BF16, E4M3, F16, F32, Q8ROW
from graphgen import torch_feature_code, torch_feature_rows, torch_fill_features

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B31, B32 = 1 << 31, 1 << 32
EXTRA = 1 << 20  # bytes past 2^32
EMPTY = 0xFFFFFFFF
SENT8 = 0x5A
SALT = 1 << 27  # added to a node id to name "the other tier's" row: more than any table here has rows


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def release():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- helpers -------------------------------------------------------------------------------------------------------------
def rows_past_4g(row_bytes):
    """Rows of a table of 2^32 + 2^20 bytes, rounded up to whole rows."""
    return -(-(B32 + EXTRA) // row_bytes)


def boundary_rows(rows, row_bytes, seed, random=300, near=70):
    """The index list of the module docstring for a table of `rows` rows of `row_bytes` bytes (numpy int64, every entry
    below rows): unsorted, repeats, a count that is no multiple of 64."""
    rs = np.random.RandomState(seed)
    parts = [np.arange(0, near)]
    for b in (B31, B32):
        r = b // row_bytes
        if r - near < rows:
            parts.append(np.arange(max(0, r - near), min(rows, r + near)))
    parts.append(rs.randint(0, rows, random))
    parts.append(np.array([rows - 1, rows - 1, 0]))
    idx = np.concatenate(parts).astype(np.int64)
    idx = np.concatenate([idx, idx[:29]])  # repeats
    idx = idx[rs.permutation(idx.size)]
    if idx.size % 64 == 0:
        idx = idx[:-1]
    assert idx.min() >= 0 and idx.max() < rows and idx.size % 64
    if rows * row_bytes > B32:
        assert (idx * row_bytes >= B32).sum() >= near and ((idx * row_bytes >= B31) & (idx * row_bytes < B32)).sum() >= near
    return idx


def i32(a):
    """Row / node ids (numpy or torch, any integer type, below 2^32) as the int32 device tensor the entry points take."""
    t = torch.as_tensor(np.asarray(a, dtype=np.int64) if not torch.is_tensor(a) else a).to("cuda", torch.int64)
    return torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)


def dev64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).cuda()


class Canaried:
    """`rows x dim` output of torch dtype `dtype` in a byte buffer filled with 0x5a: 256 bytes of canary on either side."""
    LEAD = 256

    def __init__(self, rows, dim, dtype):
        self.nbytes = rows * dim * torch.empty(0, dtype=dtype).element_size()
        self.flat = torch.full((self.LEAD + self.nbytes + self.LEAD,), SENT8, dtype=torch.uint8, device="cuda")
        self.t = self.flat[self.LEAD:self.LEAD + self.nbytes].view(dtype).view(rows, dim)

    def canaries_intact(self):
        return bool((self.flat[:self.LEAD] == SENT8).all()) and bool((self.flat[self.LEAD + self.nbytes:] == SENT8).all())

    def row_bytes_view(self):
        return self.flat[self.LEAD:self.LEAD + self.nbytes].view(self.t.shape[0], -1)

    def reset(self):
        self.flat.fill_(SENT8)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_gather(out, want, what):
    assert out.canaries_intact(), f"{what}: bytes outside the output were written"
    assert same_bytes(out.t, want), f"{what}: {int((out.t != want).any(dim=1).sum())} of {want.shape[0]} rows differ"


def big_table(row_bytes, dtype, rows=None, first_row=0):
    es = torch.empty(0, dtype=dtype).element_size()
    rows = rows_past_4g(row_bytes) if rows is None else rows
    return torch_fill_features(torch.empty((rows, row_bytes // es), dtype=dtype, device="cuda"), first_row=first_row)


# ---- plain gathers from a large table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes,dtype,rows", [(512, torch.float32, None), (400, torch.float32, 1 << 24),
                                                  (100, torch.uint8, None)], ids=["512B-f32", "400B-f32", "100B-u8"])
def test_extract_and_gather_scatter_from_a_table_past_4_gib(ops, row_bytes, dtype, rows):
    """ggms_extract and ggms_gather_scatter (source index): 512-byte rows move as 16-byte chunks and the boundaries fall
    between rows; a 400-byte row straddles each boundary; 100-byte uint8 rows move as 4-byte chunks.  The 400-byte table
    has 2^24 rows (6.7 GB) and also serves ggms_mock_extract with 24 mask bits: masked rows reach past 2^32 bytes."""
    table = big_table(row_bytes, dtype, rows)
    rows, dim = table.shape
    assert rows * row_bytes > B32
    if row_bytes == 400:
        assert any(r * 400 < b < (r + 1) * 400 for b in (B31, B32) for r in [b // 400])  # straddling rows exist
    idx = boundary_rows(rows, row_bytes, seed=row_bytes)
    t_idx = i32(idx)
    want = torch_feature_rows(dev64(idx), dim, dtype)
    n = idx.size
    out = Canaried(n, dim, dtype)
    ops.extract(table, t_idx, out=out.t)
    check_gather(out, want, "extract")
    out.reset()
    ops.gather_scatter(out.t, table, t_idx, None)
    check_gather(out, want, "gather_scatter")
    # the count on the device, below the bound: the rows past it stay untouched
    out.reset()
    m = n - 37
    ops.gather_scatter(out.t, table, t_idx, None, num=n, num_dev=torch.tensor([m], dtype=torch.int64, device="cuda"))
    assert out.canaries_intact() and same_bytes(out.t[:m], want[:m]) and bool((out.row_bytes_view()[m:] == SENT8).all())
    if rows == 1 << 24:
        bits = 24
        high = np.random.RandomState(1).randint(0, 1 << (32 - bits), n).astype(np.int64) << bits
        high[::5] = 0
        out.reset()
        ops.mock_extract(table, i32(idx | high), bits, out=out.t)
        check_gather(out, want, "mock_extract")
    assert ops.device_status() == 0


def test_long_rows_from_a_table_past_4_gib(ops):
    """Rows of 8192 16-byte chunks (131 072 bytes) go to k_gather_long_rows, one workgroup per row: 32 768 + 8 rows."""
    row_bytes, dtype = 131_072, torch.float32
    table = big_table(row_bytes, dtype, rows=32_768 + 8)
    rows, dim = table.shape
    near = np.concatenate([np.arange(0, 3), np.arange(16_384 - 3, 16_384 + 3), np.arange(32_768 - 3, 32_768 + 8)])
    idx = np.concatenate([near, np.random.RandomState(2).randint(0, rows, 9), near[:4]])
    idx = idx[np.random.RandomState(3).permutation(idx.size)]
    assert idx.size % 64 and idx.max() == rows - 1
    want = torch_feature_rows(dev64(idx), dim, dtype)
    out = Canaried(idx.size, dim, dtype)
    ops.extract(table, i32(idx), out=out.t)
    check_gather(out, want, "extract, long rows")
    out.reset()
    ops.gather_scatter(out.t, table, i32(idx), None)
    check_gather(out, want, "gather_scatter, long rows")
    assert ops.device_status() == 0


# ---- converting gathers from a large table ---------------------------------------------------------------------------------
def q8row_table(rows, dim):
    """A Q8ROW table on the device: codes and pad bytes from the feature code, a finite scale (+- 1/256 .. 4, the sign by
    row parity) and bias (-256 .. 256 in steps of 1/8) per row, both functions of the row number alone."""
    stride = ff.stride(dim)
    t = torch_fill_features(torch.empty((rows, stride), dtype=torch.uint8, device="cuda"))
    words = t.view(-1).view(torch.float32).view(rows, stride // 4)
    step = 1 << 22
    for lo in range(0, rows, step):
        r = torch.arange(lo, min(rows, lo + step), dtype=torch.int64, device="cuda")
        scale = (torch_feature_code(r, 10) + 1).to(torch.float32) / 256.0
        words[lo:lo + step, stride // 4 - 2] = torch.where(r % 2 == 1, -scale, scale)
        words[lo:lo + step, stride // 4 - 1] = (torch_feature_code(r + (1 << 40), 12) - 2048).to(torch.float32) / 8.0
    return t


CONVERT = [(F16, F32, 128), (F32, BF16, 128), (E4M3, F16, 100), (Q8ROW, F32, 128)]


@pytest.mark.parametrize("src_dt,out_dt,dim", CONVERT, ids=[f"{ff.NAMES[s]}-{ff.NAMES[o]}-dim{d}" for s, o, d in CONVERT])
def test_converting_gather_from_a_table_past_4_gib(ops, src_dt, out_dt, dim):
    """ggms_gather_scatter_convert: what a row must decode to comes from the feat_formats yardsticks applied to the
    gathered rows' STORED bytes, read back with torch indexing.  Q8ROW rows are 136 bytes apart: one row has its codes
    below 2^31 bytes and its scale / bias trailer above."""
    if src_dt == Q8ROW:
        row_bytes = ff.stride(dim)
        table = q8row_table(rows_past_4g(row_bytes), dim)
    else:
        es = {F16: 2, F32: 4, E4M3: 1}[src_dt]
        row_bytes = dim * es
        table = big_table(row_bytes, {F16: torch.float16, F32: torch.float32, E4M3: torch.uint8}[src_dt])
        if src_dt == E4M3:
            table = table.view(torch.float8_e4m3fn)
    rows = table.shape[0]
    idx = boundary_rows(rows, row_bytes, seed=row_bytes + out_dt)
    if src_dt == Q8ROW:  # the row whose trailer starts exactly at 2^31
        assert (B31 // row_bytes) * row_bytes + dim == B31 and B31 // row_bytes in idx
    stored = table.view(torch.uint8).view(rows, row_bytes)[dev64(idx)].cpu().numpy()
    if src_dt == Q8ROW:
        value = ff.decode_f32(stored[:, :dim], stored[:, row_bytes - 8:row_bytes - 4].copy().view(np.float32)[:, 0],
                              stored[:, row_bytes - 4:].copy().view(np.float32)[:, 0])
        assert np.isfinite(value).all()
        want, nan = ff.from_f32(np.ascontiguousarray(value), out_dt), np.zeros(value.shape, bool)
    elif src_dt == E4M3:
        want, nan = ff.decode_bits(stored, E4M3, out_dt), np.isnan(ff.truth(E4M3)[stored])
        assert nan.any()  # (0x7f and 0xff are codes like any other)
    else:
        bits = np.ascontiguousarray(stored).view(ff.BITS[src_dt])
        want, nan = ff.convert_bits(bits, src_dt, out_dt), np.zeros(bits.shape, bool)
    n = idx.size
    for scatter in (False, True):
        out = Canaried(n + (50 if scatter else 0), dim, ff.TORCH[out_dt])
        dst = np.random.RandomState(5).permutation(n + 50)[:n] if scatter else np.arange(n)
        ops.gather_scatter_convert(out.t, table, i32(idx), i32(dst) if scatter else None, src_dtype=src_dt)
        assert out.canaries_intact()
        got = out.t.view(ff.TORCH_BITS[out_dt]).cpu().numpy().view(ff.BITS[out_dt])
        ff.assert_bits(got[dst], want, nan, f"scatter={scatter}", dt=out_dt, codes=stored[:, :dim] if src_dt in (E4M3, Q8ROW) else None)
        untouched = np.ones(got.shape[0], bool)
        untouched[dst] = False
        assert (out.row_bytes_view().cpu().numpy()[untouched] == SENT8).all()
    assert ops.device_status() == 0


# ---- the locators, one large tier each ---------------------------------------------------------------------------------------
ROW, DIM = 512, 128  # the locators' row shape: f32, 16-byte chunks


def small_rows(ids):
    return torch_feature_rows(dev64(ids), DIM, torch.float32)


def test_partition_gather_with_one_shard_past_4_gib(ops):
    """ggms_gather_scatter_partition, P = 2: slot s lies in shard s % 2 at row s / 2.  Shard 0 is large (row r holds node
    r's row), shard 1 has 1000 rows (row r: node r + SALT)."""
    big = big_table(ROW, torch.float32)
    R = big.shape[0]
    small = small_rows(np.arange(1000) + SALT)
    r0 = boundary_rows(R, ROW, seed=11)
    r1 = np.random.RandomState(12).randint(0, 1000, 100)
    slots = np.concatenate([2 * r0, 2 * r1 + 1])
    want_ids = np.concatenate([r0, r1 + SALT])
    p = np.random.RandomState(13).permutation(slots.size)
    slots, want_ids = slots[p], want_ids[p]
    assert slots.size % 64 and slots.max() < 1 << 31
    ptab = ops.part_pointer_table([big, small])
    n = slots.size
    dst = np.random.RandomState(14).permutation(n + 50)[:n]
    out = Canaried(n + 50, DIM, torch.float32)
    ops.gather_scatter_partition(out.t, ptab, 2, i32(slots), i32(dst))
    assert out.canaries_intact() and same_bytes(out.t[dev64(dst)], small_rows(want_ids))
    untouched = torch.ones(n + 50, dtype=torch.bool, device="cuda")
    untouched[dev64(dst)] = False
    assert bool((out.row_bytes_view()[untouched] == SENT8).all())
    assert ops.device_status() == 0


@pytest.mark.parametrize("large", ["hit", "host", "no-table"])
def test_extract_cached_with_one_tier_past_4_gib(ops, large):
    """ggms_extract_cached.  hit: nodes 0 .. 999 miss (host row v holds node v + SALT), node v >= 1000 lies in cache slot
    v - 1000 of a cache past 4 GiB.  host: the host table is large (a device tensor stands in for it, as in
    test_partition_cache_paths), every seventh node below 7000 is cached (slot v / 7, holding node v + SALT).
    no-table: slot = node id in the large cache."""
    big_first = {"hit": 1000, "host": 0, "no-table": 0}[large]
    big = big_table(ROW, torch.float32, first_row=big_first)
    R = big.shape[0]
    rs = np.random.RandomState(21)
    miss = torch.full((1,), 5, dtype=torch.int64, device="cuda")  # the counter is added to (set to 0 without a table)
    if large == "hit":
        N = R + 1000
        table = torch.arange(-1000, R, dtype=torch.int64, device="cuda")
        table[:1000] = EMPTY
        host = small_rows(np.arange(1000) + SALT)
        nodes = np.concatenate([boundary_rows(R, ROW, seed=22) + 1000, rs.randint(0, 1000, 90)])
        expect = lambda v: (np.where(v < 1000, v + SALT, v), 5 + int((v < 1000).sum()))  # noqa: E731
        cache, t_table = big, i32(table)
    elif large == "host":
        N = R
        table = torch.full((N,), EMPTY, dtype=torch.int64, device="cuda")
        table[0:7000:7] = torch.arange(1000, dtype=torch.int64, device="cuda")
        cache = small_rows(np.arange(0, 7000, 7) + SALT)
        host = big
        nodes = np.concatenate([boundary_rows(R, ROW, seed=23), np.arange(0, 7000, 7)[rs.randint(0, 1000, 90)]])
        is_hit = lambda v: (v < 7000) & (v % 7 == 0)  # noqa: E731
        expect = lambda v: (np.where(is_hit(v), v + SALT, v), 5 + int((~is_hit(v)).sum()))  # noqa: E731
        t_table = i32(table)
    else:
        cache, host, t_table = big, None, None
        nodes = boundary_rows(R, ROW, seed=24)
        expect = lambda v: (v, 0)  # noqa: E731
    nodes = nodes[rs.permutation(nodes.size)]
    if nodes.size % 64 == 0:
        nodes = nodes[:-1]
    want_ids, want_miss = expect(nodes)
    out = Canaried(nodes.size, DIM, torch.float32)
    ops.extract_cached(out.t, i32(nodes), t_table, ops.part_pointer_table([cache]), 0, host, num_miss=miss)
    check_gather(out, small_rows(want_ids), f"extract_cached, large {large}")
    assert int(miss.item()) == want_miss
    assert ops.device_status() == 0


@pytest.mark.parametrize("large", ["replica", "remote", "host"])
def test_extract_tiered_with_one_tier_past_4_gib(ops, large):
    """ggms_extract_tiered, P = 2, this GPU is shard 0.  Nodes lie in four consecutive ranges: host (row = node id),
    replica (slot = position in the range), remote shard 1 and local shard 0 (slots behind the replica's, odd / even).
    The range of the tier under test has as many nodes as a table past 4 GiB has rows, the others have 500; every tier's
    rows hold node + k * SALT with a k of its own, so a row from the wrong tier is a wrong row.  The four counters
    {host, remote, local, replica} are added to."""
    Rbig = rows_past_4g(ROW)
    size = dict(host=500, replica=500, remote=500, local=500)
    size[large] = Rbig
    k = dict(host=0, remote=1, local=2, replica=3)
    start, at = {}, 0
    for tier in ("host", "replica", "remote", "local"):
        start[tier], at = at, at + size[tier]
    N = at
    tiers = {t: torch_fill_features(torch.empty((size[t], DIM), dtype=torch.float32, device="cuda"),
                                    first_row=start[t] + k[t] * SALT) for t in size}
    num_replica = size["replica"]
    table = torch.full((N,), EMPTY, dtype=torch.int64, device="cuda")
    table[start["replica"]:start["replica"] + size["replica"]] = torch.arange(size["replica"], device="cuda")
    table[start["remote"]:start["remote"] + size["remote"]] = num_replica + 2 * torch.arange(size["remote"], device="cuda") + 1
    table[start["local"]:start["local"] + size["local"]] = num_replica + 2 * torch.arange(size["local"], device="cuda")
    assert int(table[table != EMPTY].max()) < 1 << 31
    rs = np.random.RandomState(31)
    nodes, salt = [], []
    for t in size:
        r = boundary_rows(size[t], ROW, seed=32) if t == large else rs.randint(0, size[t], 60)
        nodes.append(start[t] + r)
        salt.append(np.full(r.size, k[t] * SALT))
    nodes, salt = np.concatenate(nodes), np.concatenate(salt)
    p = rs.permutation(nodes.size)
    nodes, salt = nodes[p], salt[p]
    if nodes.size % 64 == 0:
        nodes, salt = nodes[:-1], salt[:-1]
    want_counts = [7 + int((salt == k[t] * SALT).sum()) for t in ("host", "remote", "local", "replica")]
    counters = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    out = Canaried(nodes.size, DIM, torch.float32)
    ptab = ops.part_pointer_table([tiers["local"], tiers["remote"]])
    ops.extract_tiered(out.t, i32(nodes), i32(table), tiers["replica"], ptab, 2, 0, tiers["host"], tier_rows=counters)
    check_gather(out, small_rows(nodes + salt), f"extract_tiered, large {large}")
    assert counters.cpu().tolist() == want_counts and sum(want_counts) == nodes.size + 28
    assert ops.device_status() == 0


# ---- the destination side ------------------------------------------------------------------------------------------------
def test_scatter_into_an_output_past_4_gib(ops):
    """dst_index rows around both boundaries of a sentinel-filled output of 2^32 + 2^20 bytes: afterwards the rows that
    are not the sentinel are exactly the destination rows (counted on the device), and they hold the right contents."""
    R = rows_past_4g(ROW)
    src = small_rows(np.arange(4096))
    out = torch.full((R, DIM), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
    dst = np.unique(boundary_rows(R, ROW, seed=41))  # destination rows are distinct ...
    dst = dst[np.random.RandomState(42).permutation(dst.size)]  # ... and unsorted
    if dst.size % 64 == 0:
        dst = dst[:-1]
    idx = np.random.RandomState(43).randint(0, 4096, dst.size)
    ops.gather_scatter(out, src, i32(idx), i32(dst))
    written = (out.view(torch.int32) != 0x5A5A5A5A).any(dim=1)
    assert int(written.sum()) == dst.size
    t_dst = dev64(dst)
    assert bool(written[t_dst].all()) and same_bytes(out[t_dst], src[dev64(idx)])
    assert ops.device_status() == 0


def test_dense_output_identity_copy_and_dynamic_cache_past_4_gib(ops):
    """A dense gather (no dst_index) of 2^20 + 65 rows of 4096 bytes from a 4096-row table into a 4.3-GB output, against
    torch's index_select; once more with the count on the device a little below the bound.  The identity copy
    (both indices NULL) of that output.  Then the dynamic cache: the batch's 2^20 + 65 DISTINCT nodes (row i was gathered
    from table row node & 4095) are published as batch `seq`; a few hundred of them, and some nodes that were not in it,
    are gathered as batch seq + 1 with the dense output as prev_feat -- slots past 2^32 bytes -- and a host table past
    4 GiB whose rows differ from prev_feat's: hits must come from prev_feat, and the miss count must be right."""
    dim, n, extra = 1024, (1 << 20) + 65, 256
    assert n * 4096 > B32
    table = torch_feature_rows(torch.arange(4096, device="cuda"), dim, torch.float32)
    g = torch.Generator(device="cuda").manual_seed(7)
    perm = torch.randperm(n + extra, device="cuda", generator=g)
    nodes, others = perm[:n], perm[n:]
    idx = nodes & 4095
    t_idx = idx.to(torch.int32)
    out = torch.full((n, dim), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
    m = n - 1000
    ops.gather_scatter(out, table, t_idx, None, num=n, num_dev=torch.tensor([m], dtype=torch.int64, device="cuda"))
    ref = table.index_select(0, idx)
    assert same_bytes(out[:m], ref[:m]) and bool((out[m:].view(torch.int32) == 0x5A5A5A5A).all())
    ops.gather_scatter(out, table, t_idx, None)
    assert same_bytes(out, ref)
    del ref
    # identity copy
    copy = torch.full((n + 1, dim), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32)
    ops.gather_scatter(copy[:n], out, None, None, num=n)
    assert same_bytes(copy[:n], out) and bool((copy[n:].view(torch.int32) == 0x5A5A5A5A).all())
    copy.view(torch.int32).fill_(0x5A5A5A5A)
    ops.gather_scatter(copy[:n], out, None, None, num=n, num_dev=torch.tensor([m], dtype=torch.int64, device="cuda"))
    assert same_bytes(copy[:m], out[:m]) and bool((copy[m:].view(torch.int32) == 0x5A5A5A5A).all())
    del copy
    torch.cuda.empty_cache()
    # dynamic cache
    N, seq = n + extra, 0x1234_5678
    host = torch_fill_features(torch.empty((N, dim), dtype=torch.float32, device="cuda"), first_row=SALT)
    stamps = torch.zeros(N, dtype=torch.int64, device="cuda")
    ops.dynamic_cache_reset(stamps)
    t_nodes = nodes.to(torch.int32)
    ops.dynamic_cache_publish(stamps, t_nodes, seq)
    assert torch.equal(stamps[nodes], (seq << 32) | torch.arange(n, dtype=torch.int64, device="cuda"))
    assert bool((stamps[others] == 0).all())
    slot_near = torch.cat([torch.arange(0, 70), torch.arange((1 << 19) - 70, (1 << 19) + 70), torch.arange((1 << 20) - 70, n)])
    slots = torch.cat([slot_near, torch.from_numpy(np.random.RandomState(8).randint(0, n, 300)), slot_near[:20]]).cuda()
    batch = torch.cat([nodes[slots], others[:100]])
    batch = batch[torch.randperm(batch.numel(), device="cuda", generator=g)]
    assert batch.numel() % 64
    hit = stamps[batch] != 0
    want = torch.where(hit[:, None], table[batch & 4095], torch_feature_rows(batch + SALT, dim, torch.float32))
    res = Canaried(batch.numel(), dim, torch.float32)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.extract_dynamic(res.t, batch.to(torch.int32), stamps, seq + 1, out, host, num_miss=miss)
    check_gather(res, want, "extract_dynamic")
    assert int(miss.item()) == 100 == int((~hit).sum())
    assert not same_bytes(table[batch & 4095], torch_feature_rows(batch + SALT, dim, torch.float32))
    assert ops.device_status() == 0


# ---- ggms_quantize_rows --------------------------------------------------------------------------------------------------
def quantize_source(rows, dim, dtype):
    """An exactly representable affine map of the feature code: f32 (code - 2^23) / 2^16 in (-128, 128) with 16 fractional
    bits, f16 (code - 1024) / 16 in [-64, 64) with 4: negative and fractional values over every FP8 exponent from the
    subnormals up."""
    t = torch_fill_features(torch.empty((rows, dim), dtype=dtype, device="cuda"))
    off, div = (float(1 << 23), float(1 << 16)) if dtype == torch.float32 else (1024.0, 16.0)
    step = max(1, (1 << 28) // dim)
    for lo in range(0, rows, step):
        t[lo:lo + step].sub_(off).div_(div)
    return t


def rows_near(rows, row_bytes_list, random=1000, near=70, seed=0):
    parts = [np.arange(0, near), np.arange(rows - near, rows), np.random.RandomState(seed).randint(0, rows, random)]
    for rb in row_bytes_list:
        for b in (B31, B32):
            r = b // rb
            if r - near < rows:
                parts.append(np.arange(max(0, r - near), min(rows, r + near)))
    return np.unique(np.concatenate(parts))


QUANT = [(torch.float32, (1 << 23) + 70, "Q8ROW"), (torch.float32, (1 << 23) + 70, "F8E4M3"),
         (torch.float16, (1 << 25) + 70, "F8E5M2")]


@pytest.mark.parametrize("src_dtype,rows,fmt", QUANT, ids=[f"{str(d)[6:]}-{f}" for d, _, f in QUANT])
def test_quantize_rows_past_4_gib(ops, src_dtype, rows, fmt):
    """F32 (4.3 GB in) -> Q8ROW and -> F8E4M3; F16 (8.6 GB in) -> F8E5M2, whose output passes 2^32 bytes too.  Against the
    CPU yardsticks on the rows around every boundary of the source and of the output, the first and last rows and 1000
    random rows."""
    dim = 128
    src = quantize_source(rows, dim, src_dtype)
    src_rb = dim * src.element_size()
    out_rb = ff.stride(dim) if fmt == "Q8ROW" else dim
    assert rows * src_rb > B32 and (fmt != "F8E5M2" or rows * out_rb > B32)
    check = rows_near(rows, [src_rb, out_rb], seed=rows % 1000)
    out_dtype = Q8ROW if fmt == "Q8ROW" else ff.TORCH[ff.CODES[fmt]]
    out = ops.quantize_rows(src, out_dtype)
    assert out.shape == (rows, out_rb)
    t_check = dev64(check)
    values = src[t_check].cpu().numpy()
    assert (values < 0).any() and (values != np.floor(values)).any() and np.isfinite(values.astype(np.float32)).all()
    got = out.view(torch.uint8)[t_check].cpu().numpy()
    if fmt == "Q8ROW":
        want = ff.cpu_q8row(values.astype(np.float32))
        assert got.tobytes() == want.tobytes(), f"{int((got != want).any(axis=1).sum())} rows differ"
    else:
        ff.assert_fp8_bytes(got, values.astype(np.float32), fmt, fmt)
        assert np.unique(got & 0x7c if fmt == "F8E5M2" else got & 0x78).size >= 8  # several exponents
    assert ops.device_status() == 0


# ---- ggms_batch_handoff --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("es,dtype", [(4, torch.int32), (8, torch.int64)], ids=["4B", "8B"])
def test_batch_handoff_of_a_segment_past_4_gib(ops, es, dtype):
    """One segment of 2^32 + 2^20 bytes + 5 elements, its count on the device, and a short second segment behind it (its
    first workgroup is 262 209 workgroups into the grid).  Behind each destination lies a canary."""
    n, pad = (B32 + EXTRA) // es + 5, 64
    src = torch.empty(n + pad, dtype=dtype, device="cuda")
    whole = (n + pad) // 1024 * 1024
    torch_fill_features(src[:whole].view(-1, 1024))
    src[whole:] = torch_feature_rows(torch.tensor([SALT + 1], device="cuda"), n + pad - whole, dtype).view(-1)
    dst = torch.full((n + pad,), 0x5A5A5A5A, dtype=dtype, device="cuda")
    n2 = 1000 + 3
    src2 = torch_feature_rows(torch.tensor([SALT], device="cuda"), n2 + pad, dtype).view(-1)
    dst2 = torch.full((n2 + pad,), 0x5A5A5A5A, dtype=dtype, device="cuda")
    ops.batch_handoff([(src, dst, torch.tensor([n], dtype=torch.int64, device="cuda")), (src2, dst2, n2)])
    assert torch.equal(dst[:n], src[:n]) and bool((dst[n:] == 0x5A5A5A5A).all())
    assert torch.equal(dst2[:n2], src2[:n2]) and bool((dst2[n2:] == 0x5A5A5A5A).all())
    assert ops.device_status() == 0
