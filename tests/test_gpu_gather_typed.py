"""ggms_gather_typed on the GPU against its statement (tests/typed_feat_ref.py), bit for bit, on hand-built typed_nodes /
base -- no sampler.  `out` and the offset words lie between guard words and are poisoned before every call: every byte up
to off[T] must be the statement's (zero rows and zero pad bytes included), every byte behind it still poison.

xgnn_amd/csrc/gather_typed.hip: a wave takes tiles of 64 rows of ONE launch's class (a class is a chunk type: plain copies
of 16 / 8 / 4 / 2 bytes, converting pairs of 8 / 4 / 2 / 1 elements); a tile is swept run by run, a run being the rows of
one type; 8 or 16 chunk loads are in flight per lane."""
import numpy as np
import pytest

import feat_formats as ff
import typed_feat_ref as ref
from feat_formats import BF16, F16, F32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_hetero import Guarded  # noqa: E402 -- the guard / poison buffer of the hetero leaf tests

NUM_NODE = 3000
GRID_CAP = 3  # GGMS_DEBUG_GRID_CAP
BAD_IDS = [NUM_NODE, NUM_NODE + 17, 0xFFFFFFFF, 0x80000000]
N_SIZES = [0, 1, 63, 64, 65, 129, 2 * 64 * 4 + 7]
# one spec per type, cycled: (dim, table dtype, delivered dtype) or None (the type has no table)
MIXED = [(3, F32, F32), (8, F16, F32), None, (129, BF16, BF16), (100, F32, F16), (4, F16, BF16), (1, F16, F16)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def table_bits(t, rows, dim, src, out):
    """Plain copies: the aperiodic hash of (t, row, column), any bits.  Converting pairs: feat_formats' table -- every
    third element a rounding, overflow or subnormal edge -- with its NaNs replaced (a NaN's payload is not specified)."""
    if src == out:
        return ref.hashed_bits(t, rows, dim, src)
    bits = ff.table_bits(src, (rows, dim), 77 + t).copy()
    bits[np.isnan(ff.to_f32(bits, src))] = ff.from_f32(np.array([0.5], np.float32), src)[0]
    return bits


def make_case(specs, counts, mode, seed, short=(), bad=0, extra=37):
    """specs / counts: per type.  mode "rank": types shuffled over the ids, a rank table; "first": types contiguous, no
    rank table.  short: types whose table is cut to half its rows (ranks beyond it: zero rows); bad: that many entries
    replaced by ids that are no node (and, without a rank table, by ids of other types)."""
    T = len(specs)
    rng = np.random.RandomState(seed)
    node_type = rng.randint(0, T, NUM_NODE).astype(np.uint8)
    if mode == "first":
        node_type.sort()
    rank = np.zeros(NUM_NODE, np.uint32)
    tables, groups = [], []
    for t, spec in enumerate(specs):
        at = np.flatnonzero(node_type == t)
        rank[at] = np.arange(at.size)
        pool = at if at.size else np.array([0])
        groups.append(pool[rng.randint(0, pool.size, counts[t])].astype(np.uint32))
        if spec is None:
            tables.append(None)
            continue
        dim, src, out = spec
        rows = at.size // 2 if t in short else at.size
        tables.append(dict(bits=table_bits(t, rows, dim, src, out), src=src, out=out, first_node=int(pool[0])))
    typed = np.concatenate(groups + [rng.randint(0, NUM_NODE, extra).astype(np.uint32)])
    n = int(sum(counts))
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    for k in range(min(bad, n)):
        typed[rng.randint(0, n)] = BAD_IDS[k % 4] if (mode == "rank" or k % 2) else rng.randint(0, NUM_NODE)
    return dict(T=T, tables=tables, typed=typed, base=base, n=n, cap=typed.size, rank=rank if mode == "rank" else None)


def device_tables(ops, tables, base_shift=0, out_dtypes=None):
    """-> (the ggms_typed_table_t array, the tensors it points into); base_shift: every table starts that many bytes
    behind a 256-byte aligned allocation."""
    dev, keep = [], []
    for tab in tables:
        if tab is None:
            dev.append(None)
            continue
        raw = torch.from_numpy(np.ascontiguousarray(tab["bits"]).view(np.uint8).reshape(-1))
        buf = torch.full((base_shift + raw.numel() + 64,), 0xC3, dtype=torch.uint8, device="cuda")
        buf[base_shift:base_shift + raw.numel()] = raw.cuda()
        t = buf[base_shift:base_shift + raw.numel()].view(ff.TORCH[tab["src"]]).view(tab["bits"].shape)
        assert t.data_ptr() % 256 == base_shift % 256
        keep.append(buf)
        dev.append(t)
    outs = [None if tab is None else ff.TORCH[tab["out"]] for tab in tables]
    firsts = [0 if tab is None else tab["first_node"] for tab in tables]
    return ops.typed_tables(dev, outs, firsts), (keep, dev)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def run(ops, case, shift=0, base_shift=0, max_nodes=None, check=True, bufs=None):
    """One call between guards.  -> the statement's (bytes, offsets), checked unless check is False (then a closure)."""
    T, cap = case["T"], case["cap"] if max_nodes is None else max_nodes
    ct, keep = device_tables(ops, case["tables"], base_shift)
    need = ops.gather_typed_out_bytes(ct, T, cap)
    assert need == ref.out_bytes(case["tables"], cap)
    out, off = bufs if bufs is not None else (Guarded(need, shift, torch.uint8), Guarded(2 * (T + 1), 2))
    t_typed, t_base = i32(case["typed"]), i32(case["base"])
    t_rank = i32(case["rank"]) if case["rank"] is not None else None
    got = ops.gather_typed(ct, T, t_typed, t_base, row_of_node=t_rank, num_node=NUM_NODE, max_nodes=cap, out=out.t,
                           offsets=off.t.view(torch.int64))
    assert got[0].data_ptr() == out.t.data_ptr()
    want, want_off = ref.gather_typed(case["tables"], case["typed"], case["base"], cap, case["rank"], NUM_NODE)
    assert want.size <= need and (want_off % 16 == 0).all()

    def verify(prefix_of=None, keep=keep):  # (the tables stay alive with the closure)
        full = want if prefix_of is None else np.concatenate([want, prefix_of[want.size:]])
        out.check(full, "out")
        off.check(want_off.view(np.uint32), "out_offset_dev")
        np.testing.assert_array_equal(t_typed.cpu().numpy().view(np.uint32), case["typed"])
        assert ops.device_status() == 0
        return want, want_off

    return verify() if check else verify


def split(n, T, seed):
    """n slots over T types, some of them empty."""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.randint(0, n + 1, T - 1))
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int64)


@pytest.mark.parametrize("T", [1, 2, 5, 32])
@pytest.mark.parametrize("n", N_SIZES)
def test_sizes_and_types(ops, n, T):
    """Every size x every type count, mixed classes and a type without a table in one call, a rank table, a few ids that
    are no node, `out` sized for more slots than the batch has."""
    specs = [MIXED[t % len(MIXED)] for t in range(T)]
    case = make_case(specs, split(n, T, n + T), "rank", seed=n * 37 + T, bad=3 if n > 10 else 0)
    want, off = run(ops, case)
    assert off[T] == want.size and (T < 3 or off[3] == off[2])  # (type 2 has no table)


BOUNDARIES = {
    "inside_a_tile": [40, 50, 39], "exactly_on_64": [64, 64, 10], "absent_in_the_middle": [70, 0, 30],
    "absent_at_the_end": [70, 30, 0], "every_slot_of_one_type": [0, 130, 0], "first_absent": [0, 1, 200]}


@pytest.mark.parametrize("mode", ["rank", "first"])
@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_type_boundaries(ops, name, mode):
    """Three types of ONE class (so that a tile holds runs of several types): rows of 12, 20 and 404 bytes in 4-byte chunks."""
    specs = [(3, F32, F32), (5, F32, F32), (101, F32, F32)]
    run(ops, make_case(specs, BOUNDARIES[name], mode, seed=len(name)))


@pytest.mark.parametrize("mode", ["rank", "first"])
def test_a_type_without_a_table_between_two_with_tables(ops, mode):
    case = make_case([(7, F16, F16), None, (7, F16, F32)], [50, 20, 50], mode, seed=5)
    want, off = run(ops, case)
    assert off.tolist() == [0, 704, 704, 704 + 1408]  # 50 x 14 = 700 -> 704: four pad bytes


@pytest.mark.parametrize("mode", ["rank", "first"])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_every_width_as_a_plain_copy(ops, dt, mode):
    """dims 1, 3, 4, 8, 100, 128, 129: chunks of 2, 4, 8 and 16 bytes, rows of fewer and of more than 8 chunks, row bytes
    that are no multiple of 16 with odd counts -- the pad bytes exist."""
    dims = [1, 3, 4, 8, 100, 128, 129]
    case = make_case([(d, dt, dt) for d in dims], [67, 33, 65, 1, 131, 70, 77], mode, seed=dt + 1)
    want, off = run(ops, case)
    ends = [int(off[t]) + c * d * ref.ES[dt] for t, (c, d) in enumerate(zip([67, 33, 65, 1, 131, 70, 77], dims))]
    assert any(e % 16 for e in ends)
    for t, e in enumerate(ends):
        assert not want[e:int(off[t + 1])].any()


PAIRS = [(s, o) for s in (F32, F16, BF16) for o in (F32, F16, BF16)]


@pytest.mark.parametrize("dims", [[100, 8, 6, 128, 7, 1, 129, 4, 3], [1, 3, 4, 8, 100, 128, 129, 100, 8]])
def test_every_dtype_pair_in_one_call(ops, dims):
    """All nine (table, delivered) pairs as nine types of one call: plain copies beside widening and narrowing gathers,
    values that round, overflow to inf and go subnormal among the sources."""
    specs = [(d, s, o) for d, (s, o) in zip(dims, PAIRS)]
    run(ops, make_case(specs, [70, 3, 64, 65, 129, 10, 66, 1, 90], "rank", seed=dims[0]))


@pytest.mark.parametrize("mode", ["rank", "first"])
def test_ids_that_are_no_node_and_ranks_beyond_the_table(ops, mode):
    """Zero rows, nothing read for them: tables 1 and 3 hold half their types' rows, 40 entries are no node of the graph
    (or, without a rank table, nodes of other types -- before and behind their group's first id)."""
    specs = [(8, F16, F16), (100, F32, F32), (5, BF16, F32), (128, F16, F32)]
    case = make_case(specs, [90, 150, 64, 100], mode, seed=9, short=(1, 3), bad=40)
    want, off = run(ops, case)
    block = want[int(off[1]):int(off[1]) + 150 * 400].reshape(150, 400)
    assert 20 < (~block.any(axis=1)).sum() < 150


@pytest.mark.parametrize("base_shift", [4, 8])
def test_table_bases_off_a_16_byte_boundary(ops, base_shift):
    """Every table starts 4 / 8 bytes behind an aligned address: the chunk narrows to what stays aligned."""
    specs = [(128, F32, F32), (128, F16, F16), (128, F16, F32), (100, F32, F16), (8, BF16, F16)]
    run(ops, make_case(specs, [65, 70, 64, 33, 129], "rank", seed=base_shift), base_shift=base_shift)


def test_out_only_4_byte_aligned(ops):
    run(ops, make_case([(128, F32, F32), (8, F16, F32), None], [65, 70, 5], "rank", seed=3), shift=4)


@pytest.mark.parametrize("cap", [1, 3])
def test_later_rounds_of_the_grid(ops, cap):
    """9 and 17 tiles per class on 1 / 3 workgroups of four waves."""
    from xgnn_amd._lib import lib
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        specs = [MIXED[t % len(MIXED)] for t in range(5)]
        run(ops, make_case(specs, split(N_SIZES[-1], 5, cap), "rank", seed=cap, bad=5))
        run(ops, make_case([(100, F32, F32), (3, F32, F32)], [700, 380], "first", seed=cap + 10))
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


def test_two_calls_in_a_row_on_the_same_buffers(ops):
    """No synchronisation in between; the second batch is the smaller one, so the first one's bytes survive behind it."""
    specs = [(100, F32, F32), None, (40, F16, F32)]
    a = make_case(specs, [200, 30, 170], "rank", seed=1, extra=0)
    b = make_case(specs, [90, 100, 40], "rank", seed=2, extra=170)
    assert a["cap"] == b["cap"]
    ct, _ = device_tables(ops, a["tables"])
    bufs = (Guarded(ops.gather_typed_out_bytes(ct, 3, a["cap"]), 0, torch.uint8), Guarded(8, 2))
    first = run(ops, a, bufs=bufs, check=False)
    second = run(ops, b, bufs=bufs, check=False)
    want_a = ref.gather_typed(a["tables"], a["typed"], a["base"], a["cap"], a["rank"], NUM_NODE)[0]
    second(prefix_of=want_a)
    del first


def test_max_nodes_clamps_the_groups(ops):
    """base words beyond max_nodes: the groups end there, nothing behind it is read."""
    case = make_case([(3, F32, F32), (8, F16, F16), (5, F32, F16)], [50, 60, 70], "rank", seed=4)
    want, off = run(ops, case, max_nodes=75)
    assert off.tolist() == [0, 608, 608 + 400, 608 + 400]


def test_the_launch_timer_rides_on_the_first_launch(ops):
    case = make_case([(100, F32, F32), (8, F16, F32)], [300, 200], "rank", seed=6)
    timer = ops.LaunchTimer().arm()
    run(ops, case)
    assert timer.elapsed_us() > 0
    timer.close()


def test_a_table_above_4_gib(ops):
    """Type 1's table is 2^32 + 2^20 bytes of 2-KiB F16 rows; rows on either side of byte 2^31 and 2^32 and the rows a
    truncated offset would land on are gathered, widened to F32 for half of the calls.  Only the touched rows are
    initialised; the statement runs on those rows alone (compacted), with the same node ids -> ranks."""
    dim, rb = 1024, 2048
    rows = -(-((1 << 32) + (1 << 20)) // rb)
    rng = np.random.RandomState(8)
    near = np.concatenate([np.arange(0, 40), (1 << 31) // rb + np.arange(-40, 40), (1 << 32) // rb + np.arange(-40, 40),
                           rng.randint(0, rows, 100), [rows - 1]])
    touched = np.unique(near)
    assert (touched * rb >= 1 << 32).sum() >= 40
    pick = touched[rng.randint(0, touched.size, 333)]
    small = ref.hashed_bits(0, 50, 6, F32)
    big_rows = ref.hashed_bits(1, rows, 1, F16)[:, 0]  # one hash per row ...
    compact = (big_rows[touched][:, None] + np.arange(dim, dtype=np.uint16)[None, :] * np.uint16(40503)).astype(np.uint16)
    compact[np.isnan(ff.to_f32(compact, F16))] = 0x3800
    big = torch.empty((rows, dim), dtype=torch.float16, device="cuda")
    big[torch.from_numpy(touched).cuda()] = torch.from_numpy(compact.view(np.int16)).cuda().view(torch.float16)
    t_small = torch.from_numpy(small.view(np.int32)).cuda().view(torch.float32)
    first1 = 50
    typed = np.concatenate([rng.randint(0, 50, 70), first1 + pick]).astype(np.uint32)
    base = np.array([0, 70, 70 + pick.size], np.uint32)
    typed_c = np.concatenate([typed[:70], first1 + np.searchsorted(touched, pick)]).astype(np.uint32)
    for out_dt in (F16, F32):
        ct = ops.typed_tables([t_small, big], [None, ff.TORCH[out_dt]], [0, first1])
        need = ops.gather_typed_out_bytes(ct, 2, typed.size)
        out, off = Guarded(need, 0, torch.uint8), Guarded(6, 2)
        ops.gather_typed(ct, 2, i32(typed), i32(base), num_node=first1 + rows, out=out.t, offsets=off.t.view(torch.int64))
        tabs = [dict(bits=small, src=F32, out=F32, first_node=0), dict(bits=compact, src=F16, out=out_dt, first_node=first1)]
        want, want_off = ref.gather_typed(tabs, typed_c, base, typed.size, None, first1 + touched.size)
        out.check(want, f"out ({ff.NAMES[out_dt]})")
        off.check(want_off.view(np.uint32), "out_offset_dev")
        assert ops.device_status() == 0
    del big
    torch.cuda.empty_cache()
