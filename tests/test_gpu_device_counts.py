"""Node-list leaves called the way the engine calls them: `num_nodes` is a worst-case bound that sizes the launch, the
real batch size lies in device memory (`*num_nodes_dev`) and is a fraction of it -- idle waves, a grid at its cap, a
ragged last tile.  numpy / the oracle is the reference, every comparison is exact.

Trap ids: nothing here reads or writes out of range whatever a kernel does wrong.  Every table, feature array, `freq` and
`stamps` has TRAPS extra nodes N .. N + TRAPS - 1 with contents of their own; nodes[n:bound] holds trap ids only and
nodes[:n] never does; every output has `bound` entries and starts as a sentinel.  A kernel that looks past the device
count then delivers a wrong VALUE: a trap's id, slot or row in an output, a counter that is too large, a freq or stamp word
of a trap that changed, a row >= n that is no longer the sentinel.

Leaf coverage of the node-list entry points (include/ggms.h) after this file and test_gpu_owner_split.py:
  ggms_count_nodes                n edges 0 / 1 / 257 / 200 000, device count, adds on top of freq
  ggms_get_miss_cache_index_dev   device count at 0 / 1 / 1023 / 65 537 of a 100 000 bound, cache ratios 0 / 0.3 / 1
  ggms_extract_cached             table, P 0 and 3, device count under a grid at its cap, rows of 16- / 4- / 2-byte chunks,
                                  the miss counter adds (table == NULL sets it to 0: gather_harness.full_cache_case)
  ggms_extract_tiered             P 4 + replica + host tier, device count, the four counters add
  ggms_extract_dynamic / _publish device count over two batches, stamps, hit count
  ggms_owner_histogram / _bucket  n edges, P 1 .. 64, every table kind, device count (test_gpu_owner_split.py)
Past 2^31 / 2^32 BYTES (test_gpu_large_offsets.py): ggms_extract, ggms_mock_extract, ggms_gather_scatter (source index,
  dst_index scatter, dense output, identity copy, long rows), ggms_gather_scatter_convert (F16 / F32 / F8E4M3 / Q8ROW
  sources), ggms_gather_scatter_partition, ggms_extract_cached (hit tier, miss tier, table == NULL), ggms_extract_tiered
  (replica, remote shard, host tier), ggms_extract_dynamic / _publish (prev_feat slots and host rows), ggms_quantize_rows
  (source and output), ggms_batch_handoff.  Past edge POSITION 2^30 and 2^31 (test_gpu_high_offset_graph.py): the khop0 /
  khop1 / khop2 / khop3 / khop_labor leaves, random walk, ggms_sample_batch (khop3, khop0), ggms_sample_batch_prefetch,
  ggms_khop_closure, ggms_link_seeds; the three weighted samplers at 2^31.
Still open: the RCCL all-to-all on more than one GPU, and P > 8 through peer pointers; E within a few thousand of 2^32,
which no test reaches (a 17 GB index array); outputs past 2^32 ROWS; bench.py's own row check, which is periodic in the
row number (test_bench_gpu.py)."""
import numpy as np
import pytest

import oracle
from feat_formats import F16, F32, TORCH, TORCH_BITS, sentinel
from gather_harness import Out, ids
from graphgen import exact_features
from test_gpu_parity import dev, host_u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TRAPS = 64
EMPTY = 0xFFFFFFFF
SENT = 0x5A5A5A5A  # what every id / index output holds before a call


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


# ---- what both device-count test files share ---------------------------------------------------------------------------
def filled(n, value=SENT):
    """n (at least one) int32 words holding the sentinel."""
    return torch.full((max(int(n), 1),), value, dtype=torch.int32, device="cuda")


def count_dev(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


def trap_nodes(rs, N, n, bound, real=None):
    """`bound` node ids: [:n] real nodes (`real`, or random ones below N, repeats included), [n:] random trap ids."""
    nodes = np.empty(bound, np.uint32)
    nodes[:n] = rs.randint(0, N, n) if real is None else real
    nodes[n:] = N + rs.randint(0, TRAPS, bound - n)
    return nodes


def cache_table(N, num_cached, seed):
    """(cached, table): table[v] = cache slot of node v or EMPTY, N + TRAPS entries; `cached` lists the cached nodes by
    slot -- the first num_cached nodes of a random ranking, then the even traps, whose slots no real node has.  The odd
    traps are uncached."""
    rank = np.random.RandomState(seed).permutation(N).astype(np.uint32)
    cached = np.concatenate([rank[:num_cached], N + np.arange(0, TRAPS, 2, dtype=np.uint32)])
    table = np.full(N + TRAPS, EMPTY, np.uint32)
    table[cached] = np.arange(cached.size, dtype=np.uint32)
    return cached, table


_FEAT = {}


def features(dim, dt):
    """(N, host bits, device tensor) of a feature table, made once per shape and never written: N real rows and TRAPS trap
    rows, none of which holds the output sentinel.  N = 200 000 at dim 32 (two disjoint batches of 70 001 fit), else
    50 000."""
    if (dim, dt) not in _FEAT:
        N = 200_000 if dim == 32 else 50_000
        if dt == F32:  # bits of small integers as floats
            bits = exact_features(N + TRAPS, dim, np.float32).view(np.uint32)
        else:  # finite positive f16 bits below the sentinel 0x5a5a
            bits = np.random.RandomState(dim).randint(0, 0x5A00, (N + TRAPS, dim)).astype(np.uint16)
        bits.setflags(write=False)
        _FEAT[(dim, dt)] = (N, bits, rows_dev(bits, dt))
    return _FEAT[(dim, dt)]


def rows_dev(bits, dt):
    """Rows of raw bits as a device tensor of dtype TORCH[dt]."""
    a = np.array(bits).view(np.int32 if dt == F32 else np.int16)  # (a copy: the tables are read-only)
    return torch.from_numpy(a).cuda().view(TORCH[dt])


def check_rows(out, n, t_feat, t_nodes, what):
    """On the device: rows [0, n) of `out` (gather_harness.Out) are the rows nodes[:n] of t_feat byte for byte; rows
    [n, bound) and both canaries still hold the sentinel."""
    bits, s = out.flat.view(TORCH_BITS[out.dt]), sentinel(out.dt)
    rows, dim = out.shape
    assert bool((bits[:out.lead] == s).all()) and bool((bits[out.lead + rows * dim:] == s).all()), \
        f"{what}: bytes outside the output were written"
    body = bits[out.lead:out.lead + rows * dim].view(rows, dim)
    assert bool((body[n:] == s).all()), f"{what}: rows past the device count were written"
    want = t_feat.view(TORCH_BITS[out.dt])[t_nodes[:n].long()]
    assert torch.equal(body[:n], want), f"{what}: rows [0, {n}) differ from feat[nodes[:{n}]]"


# ---- ggms_count_nodes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound,n", [(0, 0), (1, 1), (257, 257), (200_000, 200_000),
                                     (1000, 0), (200_000, 257), (4134, 4097)])
def test_count_nodes(ops, bound, n):
    """freq[nodes[i]] += 1 for i < n, on top of whatever freq held: half of the batch is ONE node (a long run of atomics
    on one word), the rest random with repeats.  bound > n: the count lies on the device."""
    N = 50_000
    rs = np.random.RandomState(bound + n)
    freq0 = rs.randint(0, 1000, N + TRAPS).astype(np.uint32)
    real = np.where(rs.rand(n) < 0.5, 12_345, rs.randint(0, N, n)).astype(np.uint32)
    nodes = trap_nodes(rs, N, n, bound, real)
    t_freq, t_nodes = dev(freq0), ids(nodes)
    num_dev = count_dev(n) if bound > n else None
    want = np.bincount(nodes[:n], minlength=N + TRAPS).astype(np.uint32)
    for call in (1, 2):
        ops.count_nodes(t_freq, t_nodes, num=bound, num_dev=num_dev)
        got = host_u32(t_freq)
        np.testing.assert_array_equal(got[N:], freq0[N:], err_msg=f"call {call}: a trap node was counted")
        np.testing.assert_array_equal(got - freq0, call * want, err_msg=f"call {call}")


# ---- ggms_get_miss_cache_index_dev -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("bound,n", [(1000, 0), (1000, 1), (100_000, 1023), (100_000, 65_537), (4134, 4097)])
def test_get_miss_cache_index_dev(ops, bound, n, ratio):
    """The split of nodes[:n] with launch, index arrays and workspace sized by the bound: totals and the leading
    num_miss / num_hit entries equal the oracle's, every entry behind them is untouched."""
    N = 50_000
    rs = np.random.RandomState(bound + n)
    _, table = cache_table(N, int(N * ratio), 3)
    nodes = trap_nodes(rs, N, n, bound)
    outs = [filled(bound) for _ in range(4)]
    ms, md, nm, hs, hd, nh = ops.get_miss_cache_index(dev(table), ids(nodes), num=bound, num_dev=count_dev(n), outs=outs)
    wms, wmd, whs, whd = oracle.get_miss_cache_index(table, nodes[:n])
    assert (int(nm.item()), int(nh.item())) == (wms.size, whs.size) and wms.size + whs.size == n
    for got, want, name in ((ms, wms, "miss src"), (md, wmd, "miss dst"), (hs, whs, "hit src"), (hd, whd, "hit dst")):
        got = host_u32(got)
        np.testing.assert_array_equal(got[:want.size], want, err_msg=name)
        assert (got[want.size:] == SENT).all(), f"{name}: entries past the total were written"


# ---- the fused gathers ----------------------------------------------------------------------------------------------------
# dim 32 f32 at bound 300 000: the gather's grid is at its 256-block cap (1024 waves of one 64-row tile each per sweep);
# 65 537 is the first count at which a wave takes a second tile, 70 001 ends in a tile of 49 rows.  (4134, 4097): rows of
# 16-, 4- and 2-byte chunks.
GATHERS = [(300_000, 0, 32, F32), (300_000, 1, 32, F32), (300_000, 65, 32, F32), (300_000, 70_001, 32, F32),
           (4134, 4097, 100, F32), (4134, 4097, 1, F32), (4134, 4097, 9, F16)]
gathers = pytest.mark.parametrize("bound,n,dim,dt", GATHERS,
                                  ids=[f"{b}-{n}-dim{d}-{'f32' if t == F32 else 'f16'}" for b, n, d, t in GATHERS])


@gathers
@pytest.mark.parametrize("P", [0, 3])
def test_extract_cached_device_count(ops, P, bound, n, dim, dt):
    """ggms_extract_cached with a table: rows nodes[:n] from P shards (0: one array) or the host table; the misses of
    nodes[:n] are ADDED to *num_miss_dev (two calls: twice)."""
    N, bits, t_feat = features(dim, dt)
    cached, table = cache_table(N, int(N * 0.4), 5)
    parts = [rows_dev(bits[cached[p::max(P, 1)]], dt) for p in range(max(P, 1))]
    ptab = ops.part_pointer_table(parts)
    nodes = trap_nodes(np.random.RandomState(n + dim), N, n, bound)
    t_nodes, t_table, num_dev = ids(nodes), dev(table), count_dev(n)
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    want_miss = int((table[nodes[:n]] == EMPTY).sum())
    for call in (1, 2):
        out = Out(bound, dim, dt)
        ops.extract_cached(out.t, t_nodes, t_table, ptab, P, t_feat, num=bound, num_dev=num_dev, num_miss=miss)
        check_rows(out, n, t_feat, t_nodes, f"extract_cached P={P} call {call}")
        assert int(miss.item()) == call * want_miss, call


@gathers
def test_extract_tiered_device_count(ops, bound, n, dim, dt):
    """ggms_extract_tiered over a replica, 4 shards and the host tier: rows of nodes[:n], and the four tier counters
    count nodes[:n] only (two calls: twice)."""
    P, me, R = 4, 1, 6000
    N, bits, t_feat = features(dim, dt)
    cached, table = cache_table(N, int(N * 0.4), 6)
    replica = rows_dev(bits[cached[:R]], dt)
    parts = [rows_dev(bits[cached[R + p::P]], dt) for p in range(P)]
    ptab = ops.part_pointer_table(parts)
    nodes = trap_nodes(np.random.RandomState(n + dim + 1), N, n, bound)
    t_nodes, t_table, num_dev = ids(nodes), dev(table), count_dev(n)
    slots = table[nodes[:n]].astype(np.int64)
    missed, shard = slots == EMPTY, (slots - R) % P
    want = [int(missed.sum()), int((~missed & (slots >= R) & (shard != me)).sum()),
            int((~missed & (slots >= R) & (shard == me)).sum()), int((slots < R).sum())]
    assert sum(want) == n
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    for call in (1, 2):
        out = Out(bound, dim, dt)
        ops.extract_tiered(out.t, t_nodes, t_table, replica, ptab, P, me, t_feat, num=bound, num_dev=num_dev,
                           tier_rows=counters)
        check_rows(out, n, t_feat, t_nodes, f"extract_tiered call {call}")
        assert counters.cpu().tolist() == [call * w for w in want], call


@gathers
def test_extract_dynamic_and_publish_device_count(ops, bound, n, dim, dt):
    """Two batches of n distinct nodes each, sharing about half: batch 1 (seq 1) misses everywhere and publishes
    stamps[nodes[i]] = (1 << 32) | i for i < n; batch 2 (seq 2) hits exactly on |cur & prev[:n]| rows, read from batch 1's
    output.  The traps' stamps (a seq nobody asks for) never change."""
    N, bits, t_feat = features(dim, dt)
    rs = np.random.RandomState(n + dim + 2)
    pool = rs.permutation(N).astype(np.uint32)
    real = [pool[:n], pool[n // 2:n // 2 + n]]
    trap_stamps = (np.uint64(0x7777) << np.uint64(32)) | np.arange(TRAPS, dtype=np.uint64)
    stamps = torch.zeros(N + TRAPS, dtype=torch.int64, device="cuda")
    ops.dynamic_cache_reset(stamps)
    stamps[N:] = torch.from_numpy(trap_stamps.view(np.int64)).cuda()
    num_dev = count_dev(n)
    prev = None
    for seq in (1, 2):
        nodes = trap_nodes(rs, N, n, bound, real[seq - 1])
        t_nodes = ids(nodes)
        want_miss = n if seq == 1 else n - np.intersect1d(real[0], real[1]).size
        miss = torch.zeros(1, dtype=torch.int64, device="cuda")
        for call in (1, 2):
            out = Out(bound, dim, dt)
            ops.extract_dynamic(out.t, t_nodes, stamps, seq, prev, t_feat, num=bound, num_dev=num_dev, num_miss=miss)
            check_rows(out, n, t_feat, t_nodes, f"extract_dynamic seq {seq} call {call}")
            assert int(miss.item()) == call * want_miss, (seq, call)
        ops.dynamic_cache_publish(stamps, t_nodes, seq, num=bound, num_dev=num_dev)
        got = stamps.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(got[N:], trap_stamps, err_msg=f"seq {seq}: a trap's stamp changed")
        np.testing.assert_array_equal(got[nodes[:n]], (np.uint64(seq) << np.uint64(32)) | np.arange(n, dtype=np.uint64))
        untouched = np.ones(N, bool)
        untouched[np.concatenate(real[:seq])] = False
        assert (got[:N][untouched] == 0).all(), f"seq {seq}: a stamp outside the batch changed"
        prev = out.t
