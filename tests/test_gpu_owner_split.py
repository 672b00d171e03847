"""ggms_owner_histogram / ggms_owner_bucket, the split behind the all-to-all feature store, against numpy: slots, counts,
bucket contents, the cursors on return -- at the block and round edges of the piece loop, for 1 .. 64 shards, every kind
of table, and with the batch size left on the device (the trap ids of test_gpu_device_counts.py keep every access in
range whatever a kernel does wrong).  Everything is an integer comparison."""
import numpy as np
import pytest

from feat_formats import F32
from gather_harness import Out, ids
from graphgen import exact_features
from test_gpu_device_counts import EMPTY, SENT, TRAPS, check_rows, count_dev, filled, trap_nodes
from test_gpu_parity import dev, host_u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = 50_000
DIM = 4  # of the meaning check


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


_FEAT = []


def feat():
    """(host rows, the same on the device): N + TRAPS rows of DIM exact float32 values, made once."""
    if not _FEAT:
        f = exact_features(N + TRAPS, DIM, np.float32)
        f.setflags(write=False)
        _FEAT.extend([f, torch.from_numpy(np.array(f)).cuda()])
    return _FEAT


# ---- the reference -------------------------------------------------------------------------------------------------------
def reference(table, nodes, P):
    """(slot, owner, counts, want_row) of a batch, in unsigned 32-bit arithmetic."""
    slot = (table[nodes] if table is not None else nodes).astype(np.uint32)
    missed = slot == EMPTY
    owner = np.where(missed, P, slot % np.uint32(P)).astype(np.int64)
    return slot, owner, np.bincount(owner, minlength=P + 1), np.where(missed, nodes, slot // np.uint32(P)).astype(np.uint32)


def check_buckets(row, pos, n, start, owner, counts, want_row, what):
    """Bucket p lies in [start[p], start[p] + counts[p]): its bucket_pos are exactly the batch rows owned by p (in any
    order), each bucket_row is the row to ask p for; together the positions are a permutation of 0 .. n - 1."""
    np.testing.assert_array_equal(np.sort(pos[:n]), np.arange(n, dtype=np.uint32), err_msg=f"{what}: bucket_pos")
    for p in range(counts.size):
        seg = slice(int(start[p]), int(start[p] + counts[p]))
        np.testing.assert_array_equal(np.sort(pos[seg]), np.flatnonzero(owner == p), err_msg=f"{what}: bucket {p}")
        np.testing.assert_array_equal(row[seg], want_row[pos[seg]], err_msg=f"{what}: rows of bucket {p}")


# ---- tables: N real nodes + TRAPS traps with slots of their own -------------------------------------------------------------
def mixed_table(frac, seed=7):
    """(table, rank, num_cached): the first frac x N nodes of a random ranking are cached at their rank; the traps are
    cached behind them (slots no real node has)."""
    rank = np.random.RandomState(seed).permutation(N).astype(np.uint32)
    num_cached = int(N * frac)
    table = np.full(N + TRAPS, EMPTY, np.uint32)
    table[rank[:num_cached]] = np.arange(num_cached, dtype=np.uint32)
    table[N:] = num_cached + np.arange(TRAPS, dtype=np.uint32)
    return table, rank, num_cached


def one_owner_table(P, r):
    """Every node cached on shard r (slot = r mod P): one LDS counter and one global cursor take every lane.  The traps
    belong to the next shard."""
    table = np.empty(N + TRAPS, np.uint32)
    table[:N] = r + P * np.random.RandomState(P + r).permutation(N).astype(np.uint32)
    table[N:] = (r + 1) % P + P * (N + np.arange(TRAPS, dtype=np.uint32))
    return table


def striped_table(P):
    """Node v belongs to bucket v mod (P + 1), the host bucket included (traps too)."""
    v = np.arange(N + TRAPS, dtype=np.uint32)
    b = v % np.uint32(P + 1)
    return np.where(b == P, np.uint32(EMPTY), b + P * (v // np.uint32(P + 1))).astype(np.uint32)


def striped_nodes(rs, P, n, bound):
    """owner[i] = i mod (P + 1): every 64-lane ballot sees every bucket."""
    i = np.arange(n, dtype=np.uint32)
    return trap_nodes(rs, N, n, bound, (P + 1) * rs.randint(0, N // (P + 1), n).astype(np.uint32) + i % np.uint32(P + 1))


def wide_table(seed=11):
    """Slots all over the unsigned 32-bit range (`%` and `/` must be unsigned), a tenth uncached; nodes 0, 1, 2 hold
    0xFFFFFFFE, 0x80000000 and 0x7FFFFFFF."""
    rs = np.random.RandomState(seed)
    table = rs.randint(0, 1 << 32, N + TRAPS, dtype=np.uint64).astype(np.uint32)
    table[table == EMPTY] = 5
    table[rs.rand(N + TRAPS) < 0.1] = EMPTY
    table[:3] = [0xFFFFFFFE, 0x80000000, 0x7FFFFFFF]
    return table


# ---- one split through the C ABI -----------------------------------------------------------------------------------------
def split_case(ops, table, P, n, bound=None, nodes=None, seed=0):
    """Histogram (twice: counts are added to) and bucket of nodes[:n]; bound: the batch size lies on the device and
    `bound` sizes the launch.  Returns what the meaning check needs."""
    rs = np.random.RandomState(seed + n + P)
    dev_count = bound is not None
    bound = n if bound is None else bound
    if nodes is None:
        nodes = trap_nodes(rs, N, n, bound)
    what = f"P={P} n={n} bound={bound}"
    t_nodes, t_table = ids(nodes), (dev(table) if table is not None else None)
    num_dev = count_dev(n) if dev_count else None
    slot, owner, counts, want_row = reference(table, nodes[:n], P)

    slots_out, t_counts = filled(bound), torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    for call in (1, 2):
        ops.owner_histogram(t_table, t_nodes, P, slots_out, t_counts, num=bound, num_dev=num_dev)
        np.testing.assert_array_equal(t_counts.cpu().numpy(), call * counts, err_msg=f"{what}: counts, call {call}")
    got = host_u32(slots_out)
    np.testing.assert_array_equal(got[:n], slot, err_msg=f"{what}: slots_out")
    assert (got[n:] == SENT).all(), f"{what}: slots_out past the count was written"

    # the buckets in a random sequence, as the store lays them out ([others | me | host]), not 0 .. P
    order = rs.permutation(P + 1)
    start = np.zeros(P + 1, np.int64)
    start[order] = np.cumsum(counts[order]) - counts[order]
    cursor, row, pos = dev(start), filled(bound), filled(bound)
    ops.owner_bucket(slots_out, t_nodes, P, cursor, row, pos, num=bound, num_dev=num_dev)
    row, pos = host_u32(row), host_u32(pos)
    assert (row[n:] == SENT).all() and (pos[n:] == SENT).all(), f"{what}: bucket entries past the count were written"
    check_buckets(row, pos, n, start, owner, counts, want_row, what)
    np.testing.assert_array_equal(cursor.cpu().numpy(), start + counts, err_msg=f"{what}: cursors on return")
    return nodes, row, pos, start, counts


def check_meaning(nodes, n, row, pos, start, counts, rank, num_cached, P):
    """What the store does with the split, on the CPU: shard p holds the rows of rank[p:num_cached:P]; a bucket's rows are
    fetched from its shard (the host bucket's from the full table) and land at bucket_pos."""
    f = feat()[0]
    shards = [f[rank[p:num_cached:P]] for p in range(P)] + [f]
    out = np.full((n, DIM), -1, np.float32)
    for p in range(P + 1):
        seg = slice(int(start[p]), int(start[p] + counts[p]))
        out[pos[seg]] = shards[p][row[seg]]
    assert out.tobytes() == f[nodes[:n]].tobytes()


# The smallest shapes at which each path starts.  A workgroup owns `per` consecutive items, a whole number of 256-item
# rounds, on a grid of at most kOwnerGrid = 256 workgroups: up to 65 536 items every workgroup does one round, 65 537
# makes `per` 512 (two rounds, 127 workgroups with an empty piece), 200 000 four rounds with a ragged last piece.
MIXED = [(0, 2), (1, 1), (63, 2), (64, 3), (65, 8), (255, 63), (256, 2), (257, 64), (65_536, 8), (65_537, 3), (200_000, 64)]


@pytest.mark.parametrize("n,P", MIXED)
def test_owner_split_mixed_table(ops, n, P):
    """40 % of the nodes cached, at the block and round edges; judged by values and by what the store makes of them."""
    table, rank, num_cached = mixed_table(0.4)
    nodes, row, pos, start, counts = split_case(ops, table, P, n)
    check_meaning(nodes, n, row, pos, start, counts, rank, num_cached, P)


@pytest.mark.parametrize("bound,n,P", [(1000, 0, 2), (4134, 4097, 3), (200_000, 300, 8), (200_000, 65_537, 64)])
def test_owner_split_device_count(ops, bound, n, P):
    """The batch size on the device, the launch sized by a bound: a grid of 256 workgroups of which two have work, and a
    bound that would make four rounds where the count makes two."""
    table, rank, num_cached = mixed_table(0.4)
    nodes, row, pos, start, counts = split_case(ops, table, P, n, bound=bound)
    check_meaning(nodes, n, row, pos, start, counts, rank, num_cached, P)


@pytest.mark.parametrize("kind,n,P,bound", [("none", 200_000, 8, None), ("all", 4097, 8, None), ("all", 65_537, 2, None),
                                            ("identity", 257, 1, None), ("identity", 65_537, 8, None),
                                            ("identity", 4097, 3, 4134)])
def test_owner_split_one_sided_tables(ops, kind, n, P, bound):
    """Nothing cached (everything in bucket P), everything cached, and table == NULL (slot = node id)."""
    table = {"none": lambda: mixed_table(0.0)[0], "all": lambda: mixed_table(1.0)[0], "identity": lambda: None}[kind]()
    *_, counts = split_case(ops, table, P, n, bound=bound)
    if kind == "none":
        assert counts[P] == n
    else:
        assert counts[P] == 0


@pytest.mark.parametrize("n,P,r", [(200_000, 8, 5), (257, 64, 63), (65_537, 2, 0)])
def test_owner_split_one_owner(ops, n, P, r):
    """Every row owned by shard r: the batch lands in one bucket."""
    *_, counts = split_case(ops, one_owner_table(P, r), P, n)
    assert counts[r] == n


@pytest.mark.parametrize("n,P", [(65_537, 64), (257, 3), (4097, 8)])
def test_owner_split_striped(ops, n, P):
    """owner[i] = i mod (P + 1): every bucket in every ballot."""
    rs = np.random.RandomState(n)
    *_, counts = split_case(ops, striped_table(P), P, n, nodes=striped_nodes(rs, P, n, n))
    assert counts.min() >= n // (P + 1)


@pytest.mark.parametrize("n,P", [(1000, 3), (65_537, 7)])
def test_owner_split_slots_above_two_to_the_31(ops, n, P):
    """Slots 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF and random ones all over the 32-bit range: owner and row are the unsigned
    remainder and quotient."""
    nodes = trap_nodes(np.random.RandomState(P), N, n, n)
    nodes[:3] = [0, 1, 2]  # the three edge slots are in the batch
    split_case(ops, wide_table(), P, n, nodes=nodes)


# ---- through the Python leaf -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_count", [False, True])
@pytest.mark.parametrize("P,me", [(1, 0), (3, 0), (3, 2), (8, 0), (8, 7)])
def test_hip_leaf_split_by_owner(ops, P, me, dev_count):
    """ggms_store.HipLeaf.split_by_owner with the bucket sequence of FeatureShards._extract_a2a: [ranks ascending
    without me | me | host], the cursors computed on the device."""
    from xgnn_amd.ggms_store import HipLeaf
    n = 4097
    bound = n + 37 if dev_count else n
    table, rank, num_cached = mixed_table(0.4)
    nodes = trap_nodes(np.random.RandomState(P + me), N, n, bound)
    order = [p for p in range(P) if p != me] + [me, P]
    row, pos, t_counts = HipLeaf().split_by_owner(dev(table), ids(nodes), bound, P,
                                                  torch.tensor(order, dtype=torch.int64, device="cuda"),
                                                  **({"num_dev": count_dev(n)} if dev_count else {}))
    _, owner, counts, want_row = reference(table, nodes[:n], P)
    np.testing.assert_array_equal(t_counts.cpu().numpy(), counts)
    start = np.zeros(P + 1, np.int64)
    start[order] = np.cumsum(counts[order]) - counts[order]
    row, pos = host_u32(row), host_u32(pos)
    check_buckets(row, pos, n, start, owner, counts, want_row, f"P={P} me={me}")
    check_meaning(nodes, n, row, pos, start, counts, rank, num_cached, P)


@pytest.mark.parametrize("dev_count", [False, True])
@pytest.mark.parametrize("with_table", [True, False])
def test_feature_shards_a2a_single_process(ops, with_table, dev_count):
    """FeatureShards in mode "a2a" with world = 1 (no collective is touched): split, local gather, host gather.  extract
    equals feat[nodes[:n]]; rows past the count stay untouched."""
    from xgnn_amd.ggms_store import FeatureShards
    f, t_feat = feat()
    n = 4097
    bound = n + 37 if dev_count else n
    nodes = trap_nodes(np.random.RandomState(int(with_table)), N, n, bound)
    if with_table:
        table, rank, num_cached = mixed_table(0.4)
        # (the traps' slots lie behind the cached nodes': their rows are in the shard, so that no row id is out of range)
        shard = torch.from_numpy(f[np.concatenate([rank[:num_cached], N + np.arange(TRAPS, dtype=np.uint32)])]).cuda()
        t_table = dev(table)  # the store's tables are int32 with -1 for an uncached node: the same bits
    else:
        shard, t_table = t_feat, None
    store = FeatureShards(shard, t_table, 1, 0, mode="a2a", host_feat=t_feat)
    out, t_nodes = Out(bound, DIM, F32), ids(nodes)
    store.extract(t_nodes, bound, out.t, num_dev=count_dev(n) if dev_count else None)
    check_rows(out, n, t_feat, t_nodes, f"a2a world=1 table={with_table} dev_count={dev_count}")
