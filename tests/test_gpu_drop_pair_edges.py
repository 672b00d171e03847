"""ggms_drop_pair_edges on the GPU against its numpy statement (tests/link_exclude_ref.py), bit for bit: row, col, every
counts word (only the edge words may change) and num_dropped, on hand-built layers -- no sampler.

xgnn_amd/csrc/drop_pair_edges.hip works on tiles of 1024 edges, 4 consecutive edges per thread, as one 16-byte vector
where row / col are 16-byte aligned and the 4 edges lie inside the layer.  The pair set is one table in the workspace for
every num_pairs (there is no second, LDS-resident form), and the compaction has no look-back (snapshot, prefix, compact:
three launches), so there is no scan patience to vary."""
import ctypes as C

import numpy as np
import pytest

import link_exclude_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 1024
BIG = 5 * TILE + 80  # five whole tiles and a partial one
INVALID = -1
GUARD = 0x5A5A5A5A
FAR = 100000  # ids no pair reaches: beyond the prefilter's bound


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_and_check(ops, src, dst, which, layers, shift=0, dropped_before=1000):
    """layers: [(row, col, n, max_edges)] -- row / col hold max_edges entries, the first n are the layer (what lies
    behind is poison).  shift: row / col start that many words behind a 16-byte boundary.  The device's result must equal
    the reference's in every compared word; -> (kept layers, dropped per layer)."""
    from xgnn_amd import _lib
    L = len(layers)
    counts = np.arange(7000, 7000 + _lib.COUNTS_WORDS(L), dtype=np.int64)  # every word distinct and non-zero
    bufs = []
    for i, (row, col, n, cap) in enumerate(layers):
        assert row.size == col.size == cap and n <= cap
        counts[_lib.COUNT_EDGES(i)] = n
        pair = []
        for a in (row, col):
            t = torch.full((shift + cap + 64,), GUARD, dtype=torch.int32, device="cuda")
            t[shift:shift + cap] = dev(a)
            pair.append(t)
        bufs.append(pair)
    rows = [r[shift:shift + cap] for (r, _), (_, _, _, cap) in zip(bufs, layers)]
    cols = [c[shift:shift + cap] for (_, c), (_, _, _, cap) in zip(bufs, layers)]
    assert all(t.data_ptr() % 16 == 4 * shift for t in rows + cols)
    t_counts = torch.from_numpy(counts.copy()).cuda()
    t_dropped = torch.full((L,), dropped_before, dtype=torch.int64, device="cuda")
    got_dropped = ops.drop_pair_edges(dev(src), dev(dst), which, rows, cols, t_counts,
                                      max_edges=[cap for *_, cap in layers], num_dropped=t_dropped)
    assert got_dropped is t_dropped
    want, want_dropped = ref.drop_pair_edges(src, dst, which, [(row[:n], col[:n]) for row, col, n, _ in layers])
    got_counts = t_counts.cpu().numpy()
    want_counts = counts.copy()
    for i in range(L):
        want_counts[_lib.COUNT_EDGES(i)] = want[i][0].size
    print(f"which {which} pairs {len(src)} layers {[n for _, _, n, _ in layers]}: dropped {want_dropped}")
    np.testing.assert_array_equal(got_counts, want_counts)  # all 3 L + 8 words
    np.testing.assert_array_equal(t_dropped.cpu().numpy(), np.array(want_dropped) + dropped_before)  # ADDED to
    for i, ((r, c), (_, _, _, cap)) in enumerate(zip(bufs, layers)):
        k = want[i][0].size
        np.testing.assert_array_equal(host_u32(r)[shift:shift + k], want[i][0], err_msg=f"row of layer {i}")
        np.testing.assert_array_equal(host_u32(c)[shift:shift + k], want[i][1], err_msg=f"col of layer {i}")
        for t in (r, c):  # nothing outside the layer's max_edges entries is written
            h = host_u32(t)
            assert (h[:shift] == GUARD).all() and (h[shift + cap:] == GUARD).all()
    assert ops.device_status() == 0
    return want, want_dropped


def make_pairs(num_pairs, seed=0):
    """An asymmetric list: sources 0 .. 99, destinations 100 .. 199, so no pair is another one's mirror."""
    rng = np.random.RandomState(100 + num_pairs + seed)
    return rng.randint(0, 100, num_pairs).astype(np.uint32), rng.randint(100, 200, num_pairs).astype(np.uint32)


def big_layer(src, dst, seed=1):
    """BIG edges.  Background: ids 0 .. 299 on both sides (below and around the prefilter's bound: they are probed and
    nearly all kept).  Planted: positives and mirrors in the first and in the last (partial) tile; tile 2 holds nothing
    but positives and mirrors; edges with a pair's id on one side and an id beyond the bound on the other."""
    rng = np.random.RandomState(seed)
    row = rng.randint(0, 300, BIG).astype(np.uint32)
    col = rng.randint(0, 300, BIG).astype(np.uint32)
    P = src.size
    def plant(at, p, mirror):
        col[at], row[at] = (dst[p], src[p]) if mirror else (src[p], dst[p])
    for j, at in enumerate([0, 1, 2, 63, 64, 255, 256, 1023, 5 * TILE, 5 * TILE + 1, BIG - 2, BIG - 1]):
        plant(at, j % P, j % 3 == 0)
    for at in range(2 * TILE, 3 * TILE):
        plant(at, at % P, at % 2 == 1)
    for j, at in enumerate(range(3 * TILE + 5, 3 * TILE + 45)):  # one side beyond the bound: never a match
        p = j % P
        if j % 2:
            col[at], row[at] = src[p], FAR + j
        else:
            col[at], row[at] = FAR + j, dst[p]
    return row, col


@pytest.mark.parametrize("which", [1, 2, 3], ids=["forward", "reverse", "both"])
@pytest.mark.parametrize("num_pairs", [1, 63, 64, 65])
def test_big_layer_equals_the_reference(ops, num_pairs, which):
    src, dst = make_pairs(num_pairs)
    row, col = big_layer(src, dst)
    want, dropped = run_and_check(ops, src, dst, which, [(row, col, BIG, BIG)])
    # the planted cases are there: first tile, last tile, the whole of tile 2 -- and the three modes differ
    keep = ref.keep_mask(row, col, ref.pair_set(src, dst, which))
    assert not keep[:TILE].all() and not keep[5 * TILE:].all() and keep[3 * TILE + 5:3 * TILE + 45].all()
    both = ref.keep_mask(row, col, ref.pair_set(src, dst, 3))
    assert not both[2 * TILE:3 * TILE].any() and (which == 3 or keep[2 * TILE:3 * TILE].any())
    assert 0 < dropped[0] < BIG


def test_three_layers_of_very_different_sizes_and_poison_behind_the_count(ops):
    """L = 3: a big layer well below its bound, a layer of 0 edges, a layer of 1 edge.  Behind every n_i lie positives:
    read as edges they would be dropped and counted."""
    src, dst = make_pairs(65)
    row, col = big_layer(src, dst, seed=2)
    cap = 3 * BIG
    prow, pcol = np.resize(dst, cap).astype(np.uint32), np.resize(src, cap).astype(np.uint32)  # poison: positives
    prow[:BIG], pcol[:BIG] = row, col
    one_r, one_c = np.resize(dst, 40).astype(np.uint32), np.resize(src, 40).astype(np.uint32)
    for first_kept in (True, False):
        r1, c1 = one_r.copy(), one_c.copy()
        if first_kept:
            r1[0] = 250  # the layer's only edge is no positive
        layers = [(prow, pcol, BIG, cap), (one_r, one_c, 0, 40), (r1, c1, 1, 40)]
        want, dropped = run_and_check(ops, src, dst, 3, layers)
        assert dropped[1] == 0 and dropped[2] == (0 if first_kept else 1) and want[1][0].size == 0


def test_layers_where_everything_matches(ops):
    """Every edge is a positive or a mirror: `both` leaves nothing, `self` the mirrors -- over several tiles, and in a
    layer of one edge (L = 1)."""
    src, dst = make_pairs(64)
    n = 3 * TILE + 7
    p = np.arange(n) % 64
    mirror = (np.arange(n) % 3) == 0
    col = np.where(mirror, dst[p], src[p]).astype(np.uint32)
    row = np.where(mirror, src[p], dst[p]).astype(np.uint32)
    want, dropped = run_and_check(ops, src, dst, 3, [(row, col, n, n)])
    assert dropped == [n] and want[0][0].size == 0
    want, dropped = run_and_check(ops, src, dst, 1, [(row, col, n, n)])
    assert dropped == [int((~mirror).sum())]
    want, dropped = run_and_check(ops, src, dst, 3, [(row[:1], col[:1], 1, 1)])
    assert dropped == [1]


def test_repeated_self_and_empty_pairs(ops):
    """Repeated pairs, a pair (u, u) under either bit, pairs holding EMPTY (they match nothing, and edges that hold EMPTY
    stay), ids of all sizes."""
    E = ref.EMPTY
    src = np.array([5, 5, 5, 9, E, 7, E, 0x7FFFFFFF, 5], np.uint32)
    dst = np.array([6, 6, 6, 9, 7, E, E, 0xFFFFFFFE, 6], np.uint32)
    rng = np.random.RandomState(3)
    n = 2 * TILE + 300
    row = rng.randint(0, 12, n).astype(np.uint32)
    col = rng.randint(0, 12, n).astype(np.uint32)
    for at, (c, r) in zip(range(100, 2300, 200), [(E, 7), (7, E), (E, E), (0x7FFFFFFF, 0xFFFFFFFE), (0xFFFFFFFE, 0x7FFFFFFF),
                                                  (9, 9), (5, 6), (6, 5), (E, 5), (0xFFFFFFFE, 0xFFFFFFFE), (9, 9)]):
        col[at], row[at] = c, r
    for which in (1, 2, 3):
        want, dropped = run_and_check(ops, src, dst, which, [(row, col, n, n)])
        kept = set(zip(want[0][1].tolist(), want[0][0].tolist()))
        assert (9, 9) not in kept and {(E, 7), (7, E), (E, E)} <= kept
        assert ((5, 6) in kept) == (which == 2) and ((6, 5) in kept) == (which == 1)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_rows_that_are_not_16_byte_aligned(ops, shift):
    """row / col start 4, 8 or 12 bytes behind a 16-byte boundary: the element-wise loads."""
    src, dst = make_pairs(65, seed=shift)
    row, col = big_layer(src, dst, seed=10 + shift)
    run_and_check(ops, src, dst, 3, [(row, col, BIG - 3, BIG), (row[:9].copy(), col[:9].copy(), 9, 9)], shift=shift)


def test_no_pairs_and_no_bits_leave_everything(ops):
    src, dst = make_pairs(65)
    row, col = big_layer(src, dst)
    for s, d, which in ((src, dst, 0), (src[:0], dst[:0], 3)):
        want, dropped = run_and_check(ops, s, d, which, [(row, col, BIG, BIG)])
        assert dropped == [0] and want[0][0].size == BIG


def test_argument_errors_launch_nothing(ops):
    from xgnn_amd._lib import COUNT_EDGES, lib
    l = lib()
    src, dst = make_pairs(65)
    row, col = big_layer(src, dst)
    t_row, t_col, t_src, t_dst = dev(row), dev(col), dev(src), dev(dst)
    counts = torch.zeros(11, dtype=torch.int64, device="cuda")
    counts[COUNT_EDGES(0)] = BIG
    dropped = torch.zeros(1, dtype=torch.int64, device="cuda")
    me = (C.c_size_t * 1)(BIG)
    need = l.ggms_drop_pair_edges_workspace_bytes(65, me, 1)
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows, cols = (C.c_void_p * 1)(t_row.data_ptr()), (C.c_void_p * 1)(t_col.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(src=ptr(t_src), dst=ptr(t_dst), n=65, which=3, row=rows, col=cols, me=me, L=1, counts=ptr(counts),
                dropped=ptr(dropped), ws=ptr(ws), wsb=need, stream=stream)
    call = lambda **kw: l.ggms_drop_pair_edges(*[kw.get(k, v) for k, v in base.items()])  # noqa: E731
    for kw in (dict(which=4), dict(L=0), dict(L=17), dict(row=None), dict(col=None), dict(me=None), dict(counts=None),
               dict(src=None), dict(dst=None), dict(ws=None), dict(wsb=need - 1), dict(row=(C.c_void_p * 1)(None))):
        assert call(**kw) == INVALID, kw
        assert l.ggms_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(t_row), row)
    np.testing.assert_array_equal(host_u32(t_col), col)
    assert int(counts[COUNT_EDGES(0)]) == BIG and int(dropped[0]) == 0 and ops.device_status() == 0
    assert call() == 0  # and the same arguments, all valid, do run
    torch.cuda.synchronize()
    assert int(counts[COUNT_EDGES(0)]) < BIG and int(dropped[0]) == BIG - int(counts[COUNT_EDGES(0)])


def test_batch_sampler_helper(ops):
    """BatchSampler.drop_pair_edges on a sampled batch: 64 ring nodes of degree 4, fanout 8 (every list whole), the
    seeds are the endpoints of 16 ring edges.  The filtered layers are the reference's filter of the sampled ones."""
    n = 64
    lists = np.array([[(v + 1) % n, (v - 1) % n, (v + 2) % n, (v - 2) % n] for v in range(n)], np.uint32)
    ip = (np.arange(n + 1) * 4).astype(np.uint32)
    g = ops.DeviceGraph(dev(ip), dev(lists.reshape(-1)))
    bs = ops.BatchSampler(g, [8, 8], 32, sample_type=ops.KHOP0, device="cuda")
    u = np.arange(0, 48, 3, dtype=np.uint32)
    seeds = np.concatenate([u, (u + 1) % n]).astype(np.uint32)  # positives u -> u + 1
    bs.sample(dev(seeds))
    before = [(host_u32(l["row"]).copy(), host_u32(l["col"]).copy()) for l in bs.result()["layers"]]
    ids = bs.seed_ids().clone()
    B = u.size
    dropped = bs.drop_pair_edges(ids[:B].contiguous(), ids[B:].contiguous(), ops.DROP_FORWARD | ops.DROP_REVERSE)
    after = bs.result()["layers"]
    want, want_dropped = ref.drop_pair_edges(host_u32(ids[:B]), host_u32(ids[B:]), 3, before)
    assert dropped.cpu().tolist() == want_dropped and want_dropped[1] == 2 * B  # the first layer holds every positive twice
    for lay, (r, c), (r0, _) in zip(after, want, before):
        np.testing.assert_array_equal(host_u32(lay["row"]), r)
        np.testing.assert_array_equal(host_u32(lay["col"]), c)
        assert r.size < r0.size
