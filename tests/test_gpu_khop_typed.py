"""khop_typed on the GPU against its numpy statement (tests/khop_typed_ref.py), bit for bit.  The leaf: every segment
length at which the kernels change route (as the first, a middle and the last segment of a list), zero fanouts, absent
types, one-type lists, R = 1 / 2 / 5 / 32, boundaries at the wave's edge, misaligned arrays, duplicate seeds, later
grid-stride rounds, positions past 2^31, an unsorted list.  The batch: both table layouts, a row of fanouts per layer,
repeated seeds, the khop_labor batch it must equal with one type, and the delivered positions and types."""
import numpy as np
import pytest

import khop_labor_ref as labor
import khop_typed_ref as ref
from xgnn_amd._lib import COUNT_DST, COUNT_EDGES, COUNT_INPUT, COUNT_SRC, COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HUB = 40_000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a, shift=0):
    """The array on the device.  uint32: shift = 1 puts it 4 bytes behind a 16-byte boundary; uint8: `shift` bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a).cuda()
    if shift:
        buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + t.numel()] = t
        t = buf[shift:shift + t.numel()]
        assert t.data_ptr() % 16 == shift * t.element_size()
    return t


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


def check_leaf(ops, g, t_et, ip, ix, et, inp, tf, salt, shift=0):
    src, dst, pos, typ, num = ops.sample_khop_typed(g, t_et, tf, dev(inp, shift), salt)
    _, wsrc, wdst, wpos, wtyp = ref.sample_layer(ip, ix, et, inp, tf, salt)
    m = int(num.item())
    assert m == wsrc.size
    np.testing.assert_array_equal(host_u32(pos, m), wpos)
    np.testing.assert_array_equal(typ.cpu().numpy()[:m], wtyp)
    np.testing.assert_array_equal(host_u32(src, m), wsrc)
    np.testing.assert_array_equal(host_u32(dst, m), wdst)
    assert ops.device_status() == 0
    return host_u32(pos, m).copy()


def segment_lengths(k):
    return sorted({0, 1, k, k + 1, 64, 65, 256, 257, 1024, 1025, HUB})


@pytest.fixture(scope="module")
def segment_graphs(ops):
    """Per fanout k, three types: for every length e a list whose FIRST segment has e entries (5 and 3 behind it), one
    whose LAST has (3 and 5 in front), one that is all one type (the middle one), one with e entries of type 0 and of
    type 2 and none between.  [64, 50, 9] and [65, 50, 9] put a boundary at positions 63 | 64 and 64 | 65.  Then a
    HUB-entry list whose sampled segments have 3 and 7 entries: routed by e_r, not by the degree."""
    made = {}

    def get(k):
        if k not in made:
            lists = []
            for e in segment_lengths(k):
                lists += [[e, 5, 3], [3, 5, e], [0, e, 0], [e, 0, e]]
            lists += [[64, 50, 9], [65, 50, 9], [63, 1, 64], [3, HUB - 10, 7]]
            ip, ix, et = ref.segment_graph(lists)
            made[k] = (ip, ix, et, ops.DeviceGraph(dev(ip), dev(ix)), dev(et))
        return made[k]
    yield get
    made.clear()


@pytest.mark.parametrize("k", [1, 10, 127])
def test_leaf_every_segment_length(ops, segment_graphs, k):
    ip, ix, et, g, t_et = segment_graphs(k)
    inp = np.arange(ip.size - 1, dtype=np.uint32)
    check_leaf(ops, g, t_et, ip, ix, et, inp, [k, 0, k], 0)            # a zero fanout in the middle
    check_leaf(ops, g, t_et, ip, ix, et, inp, [k, k, k], 0x4329F67E)   # the one-type lists and the hub's long segment
    check_leaf(ops, g, t_et, ip, ix, et, inp, [0, 3, 0], 5)
    check_leaf(ops, g, t_et, ip, ix, et, inp, [k, 2, 1, 9], 7)         # R = 4: a type that no list holds


def random_typed_graph(rng, n, R, max_deg=300, hubs=3, absent=None, hub_deg=(1100, 3000)):
    """Random lists (some empty, `hubs` of hub_deg entries, every tenth all one type), neighbour ids below n."""
    deg = rng.randint(0, max_deg, n)
    deg[rng.randint(0, n, max(1, n // 40))] = 0
    deg[rng.permutation(n)[:hubs]] = rng.randint(hub_deg[0], hub_deg[1], hubs)
    ip = np.zeros(n + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, n, int(ip[-1])).astype(np.uint32)
    w = rng.random_sample(R) + 0.05
    if absent is not None and R > 1:
        w[absent] = 0
    et = ref.sorted_types(ip, rng, R, w / w.sum())
    for v in range(0, n, 10):
        et[ip[v]:ip[v + 1]] = et[ip[v]] if ip[v] < ip[v + 1] else 0
    return ip, ix, et


@pytest.mark.parametrize("R", [1, 2, 5, 32])
def test_leaf_type_counts(ops, R):
    rng = np.random.RandomState(R)
    ip, ix, et = random_typed_graph(rng, 600, R, absent=(R // 2 + 1) % R)  # a type that no list holds
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    inp = rng.randint(0, 600, 700).astype(np.uint32)
    inp[650:] = inp[:50]  # duplicate seeds get the same edges
    tf = rng.randint(0, 6, R)
    tf[0], tf[R // 2], tf[-1] = 127 if R > 1 else 10, (0 if R > 2 else tf[R // 2]), max(tf[-1], 1)
    pos = check_leaf(ops, g, t_et, ip, ix, et, inp, tf.tolist(), 0xC0FFEE + R)
    again = check_leaf(ops, g, t_et, ip, ix, et, inp, tf.tolist(), 0xC0FFEE + R)
    assert np.array_equal(pos, again)
    if R == 1:  # exactly khop_labor with fanout k_0
        src, dst, num = ops.sample_khop_labor(g, dev(inp), int(tf[0]), 0xC0FFEE + R)
        s2, d2, _, _, n2 = ops.sample_khop_typed(g, t_et, tf.tolist(), dev(inp), 0xC0FFEE + R)
        m = int(num.item())
        assert m == int(n2.item())
        assert torch.equal(src[:m], s2[:m]) and torch.equal(dst[:m], d2[:m])


@pytest.mark.parametrize("shift", [1, 3])
def test_leaf_misaligned_arrays(ops, shift):
    """edge_type 1 and 3 bytes behind a 16-byte boundary; indptr, indices and the seeds 4 bytes behind one."""
    rng = np.random.RandomState(8 + shift)
    ip, ix, et = random_typed_graph(rng, 400, 5)
    g, t_et = ops.DeviceGraph(dev(ip, 1), dev(ix, 1)), dev(et, shift)
    check_leaf(ops, g, t_et, ip, ix, et, rng.permutation(400).astype(np.uint32), [3, 0, 10, 1, 127], 21, shift=1)


def test_leaf_empty_input(ops):
    ip, ix, et = ref.segment_graph([[3, 2]])
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert int(ops.sample_khop_typed(g, t_et, [1, 1], z, 1)[4].item()) == 0


def test_leaf_unsorted_list_stays_inside_the_list(ops):
    """A violated precondition (and types >= R): which edges come out is unspecified, but every position lies in its
    seed's list, no seed emits more than K edges, and the run completes with a clean status."""
    rng = np.random.RandomState(6)
    deg = rng.randint(0, 1500, 300)
    ip = np.zeros(301, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, 1 << 20, int(ip[-1])).astype(np.uint32)
    et = rng.randint(0, 7, int(ip[-1])).astype(np.uint8)  # unsorted, and 5 / 6 are out of range for R = 5
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    tf = [3, 0, 10, 1, 4]
    src, dst, pos, typ, num = ops.sample_khop_typed(g, t_et, tf, dev(np.arange(300, dtype=np.uint32)), 3)
    m = int(num.item())
    s, p, d = host_u32(src, m).astype(np.int64), host_u32(pos, m).astype(np.int64), host_u32(dst, m)
    assert m <= 300 * sum(tf) and ((p >= ip[s]) & (p < ip[s + 1])).all() and (ix[p] == d).all()
    assert (np.diff(s) >= 0).all() and np.bincount(s, minlength=300).max() <= sum(tf)
    assert (typ.cpu().numpy()[:m] < 5).all()
    assert ops.device_status() == 0


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(3, request.param)  # GGMS_DEBUG_GRID_CAP
    yield request.param
    lib().ggms_debug_set_knob(3, -1)
    assert ops.device_status() == 0


@pytest.mark.parametrize("R", [1, 5])
def test_leaf_later_grid_rounds(ops, cap, R):
    """3401 seeds (13 x 256 + an odd remainder) under a grid cap of 1 and 3 workgroups: k_typed_bounds takes 256 / G seeds
    per workgroup round (G = 1 with one type: 256, the largest unit), k_typed_select 4 (a wave each, the next seed's
    count carried over), k_typed_hub one listed seed (14 of them: LDS reused behind the closing barrier)."""
    rng = np.random.RandomState(cap)
    ip, ix, et = random_typed_graph(rng, 3401, R, max_deg=120, hubs=14, hub_deg=(6000, 9000))
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    tf = [10] if R == 1 else [4, 2, 2, 1, 3]
    check_leaf(ops, g, t_et, ip, ix, et, rng.permutation(3401).astype(np.uint32), tf, 0xABCD)


def test_leaf_positions_past_2_31(ops):
    """graphgen.high_offset_csr at 2^31: the hub's list has edge position 2^31 in its middle, half of the real nodes lie
    above it.  The reference works on the shifted graph (the filler at degree 0); its positions are shifted back."""
    from graphgen import high_offset_csr, high_offset_table
    g = high_offset_csr(1 << 31, seed=31)
    try:
        ip, ix = g.indptr_shifted, g.indices_shifted
        et = ref.sorted_types(ip, np.random.RandomState(31), 4)
        graph = ops.DeviceGraph(dev(g.indptr), g.indices)
        t_et = high_offset_table(g, et)
        rng = np.random.RandomState(5)
        lo, hi = rng.permutation(g.below)[:150], rng.permutation(g.above)[:150]
        inp = np.concatenate([[g.hub, g.hub], lo, hi]).astype(np.uint32)
        for tf in ([2, 0, 5, 1], [25, 25, 25, 25]):
            src, dst, pos, typ, num = ops.sample_khop_typed(graph, t_et, tf, dev(inp), 0xC0FFEE)
            _, wsrc, wdst, wpos, wtyp = ref.sample_layer(ip, ix, et, inp, tf, 0xC0FFEE)
            ea, fill = g.head.size, g.tail_start - g.head.size
            wpos = np.where(wpos >= ea, wpos.astype(np.int64) + fill, wpos).astype(np.uint32)
            m = int(num.item())
            assert m == wsrc.size and (wpos >= 1 << 31).any() and (wpos < 1 << 31).any()
            np.testing.assert_array_equal(host_u32(pos, m), wpos)
            np.testing.assert_array_equal(typ.cpu().numpy()[:m], wtyp)
            np.testing.assert_array_equal(host_u32(src, m), wsrc)
            np.testing.assert_array_equal(host_u32(dst, m), wdst)
        assert ops.device_status() == 0
    finally:
        del g, graph, t_et
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_leaf_refuses_bad_arguments_on_the_device(ops):
    from xgnn_amd._lib import GgmsError
    ip, ix, et = ref.segment_graph([[3, 2, 4]])
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    inp = dev(np.zeros(4, np.uint32))
    for tf in ([0, 0, 0], [1, 128, 1], [], [1] * 33):
        with pytest.raises(GgmsError, match="invalid argument"):
            ops.sample_khop_typed(g, t_et, tf, inp, 1)
    sharded = ops.DeviceGraph(None, None, part_indptr=[dev(ip), dev(ip)], part_indices=[dev(ix), dev(ix)], num_cache_node=1)
    with pytest.raises(GgmsError, match="invalid argument"):
        ops.sample_khop_typed(sharded, t_et, [1, 1, 1], inp, 1)
    assert ops.device_status() == 0


# ---- the batch -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_graph(ops):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    et = ref.sorted_types(ip, np.random.RandomState(2), 4, [0.6, 0.0, 0.37, 0.03])  # type 1 absent, type 3 rare
    return ip, ix, et, ops.DeviceGraph(dev(ip), dev(ix)), dev(et)


def batch_seeds(rng, num_node=20_000):
    """301 seeds of which 40 are repeats."""
    seeds = rng.permutation(num_node)[:301].astype(np.uint32)
    seeds[261:] = seeds[:40]
    return seeds


def check_batch(bs, got, c, want, what=""):
    L = bs.L
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"], err_msg=what)
    assert c[COUNT_INPUT(L)] == want["input_nodes"].size and c[COUNT_STATUS(L)] == 0
    for i in range(L):
        gl, wl = got["layers"][i], want["layers"][i]
        assert (c[COUNT_EDGES(i)], c[COUNT_SRC(i)], c[COUNT_DST(i)]) == (wl["row"].size, wl["num_src"], wl["num_dst"]), (what, i)
        for key in ("row", "col", "eid"):
            np.testing.assert_array_equal(host_u32(gl[key]), wl[key], err_msg=f"{what} {key} layer {i}")
        np.testing.assert_array_equal(gl["etype"].cpu().numpy(), wl["etype"], err_msg=f"{what} etype layer {i}")
    np.testing.assert_array_equal(host_u32(bs.seed_ids()), want["seed_local"], err_msg=what)


TYPE_FANOUTS = {"L1": [[3, 2, 0, 2]], "L2": [[3, 2, 0, 2], [0, 1, 4, 1]], "L3": [[2, 0, 1, 1], [1, 1, 1, 1], [4, 0, 0, 3]]}


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("layers", ["L1", "L2", "L3"])
def test_batch_equals_the_reference(ops, batch_graph, layers, direct):
    ip, ix, et, g, t_et = batch_graph
    tfs = TYPE_FANOUTS[layers]  # another row of fanouts for every layer
    bs = ops.TypedBatchSampler(g, t_et, tfs, 301, direct_table=direct, max_seeds=301)
    assert bs.fanouts == [sum(row) for row in tfs]
    rng = np.random.RandomState(len(tfs))
    for rep in range(2):  # the second batch finds the first one's words in both tables
        seeds = batch_seeds(rng)
        salt = labor.batch_salt(42, rep, 17)
        bs.sample(dev(seeds), salt)
        got = bs.result()
        want = ref.sample_batch(ip, ix, et, seeds, tfs, salt)
        check_batch(bs, got, bs.counts.cpu().tolist(), want, f"rep {rep}")
        # the positions and types are those of the edges
        nodes = host_u32(got["input_nodes"]).astype(np.int64)
        for la in got["layers"]:
            eid, row, col = (host_u32(la[key]).astype(np.int64) for key in ("eid", "row", "col"))
            assert (et[eid] == la["etype"].cpu().numpy()).all() and (ix[eid] == nodes[row]).all()
            assert (eid >= ip[nodes[col]]).all() and (eid < ip[nodes[col] + 1]).all()


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_batch_with_one_type_equals_the_khop_labor_batch(ops, batch_graph, direct):
    """num_type = 1: ggms_sample_batch(GGMS_KHOP_LABOR) on the same graph, the project's existing kernels, gives the same
    batch."""
    ip, ix, _, g, _ = batch_graph
    t_et = torch.zeros(ix.size, dtype=torch.uint8, device="cuda")
    fanouts = [3, 4, 5]
    seeds = batch_seeds(np.random.RandomState(3))
    tb = ops.TypedBatchSampler(g, t_et, [[f] for f in fanouts], 301, direct_table=direct, max_seeds=301)
    lb = ops.BatchSampler(g, fanouts, 301, sample_type=ops.KHOP_LABOR, direct_table=direct)
    tb.sample(dev(seeds), 0xDA2897D6)
    lb.sample(dev(seeds), labor_salt=0xDA2897D6)
    a, b = tb.result(), lb.result()
    np.testing.assert_array_equal(host_u32(a["input_nodes"]), host_u32(b["input_nodes"]))
    assert tb.counts.cpu().tolist() == lb.counts.cpu().tolist()
    nodes = host_u32(a["input_nodes"]).astype(np.int64)
    for la, lb_ in zip(a["layers"], b["layers"]):
        np.testing.assert_array_equal(host_u32(la["row"]), host_u32(lb_["row"]))
        np.testing.assert_array_equal(host_u32(la["col"]), host_u32(lb_["col"]))
        assert (la["etype"] == 0).all()
        assert (ix[host_u32(la["eid"]).astype(np.int64)] == nodes[host_u32(la["row"]).astype(np.int64)]).all()
