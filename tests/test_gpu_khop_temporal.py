"""khop_temporal on the GPU against its numpy statement (tests/khop_temporal_ref.py), bit for bit.  The leaf: every
prefix length at which the kernels change route (with the list ending there and with a long ineligible tail behind it),
cuts at every edge of the strict comparison, parallel edges, duplicate seeds, both picks, misaligned arrays, later
grid-stride rounds, positions past 2^31.  The batch: the cut rule on both table layouts, stale and wrapped stamps, the
khop_labor batch it must equal without cuts, and the no-leak property on a clustered graph."""
import numpy as np
import pytest

import khop_labor_ref as labor
import khop_temporal_ref as ref
from test_khop_temporal_host import check_no_leak
from xgnn_amd._lib import COUNT_DST, COUNT_EDGES, COUNT_INPUT, COUNT_SRC, COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

INF = ref.INF
NUM_ID = 1 << 20  # neighbour ids of the leaf graphs (a leaf never follows them)
CUT = 1000        # the leaf graphs' cut: eligible times are 1 .. 999, the tails' 1000 .. 1999
HUB = 40_000
PICKS = [ref.UNIFORM, ref.RECENT]
pick_ids = ["uniform", "recent"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a, shift=0):
    """The array on the device; shift = 1: in a buffer that starts 4 bytes behind a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a).cuda()
    if shift:
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[1:1 + t.numel()] = t
        t = buf[1:1 + t.numel()]
        assert t.data_ptr() % 16 == 4
    return t


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


def timed_graph(lists):
    """lists: (ids, times) per node -> (indptr, indices, edge_time)."""
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum([len(x[0]) for x in lists])
    ix = np.concatenate([np.asarray(x[0], np.uint32) for x in lists])
    et = np.concatenate([np.asarray(x[1], np.uint32) for x in lists])
    assert ix.size == et.size == ip[-1]
    return ip, ix, et


def prefix_list(rng, e, d):
    """A list of d entries whose first e lie before CUT (sorted, with ties), the others at or after it."""
    ids = rng.randint(0, NUM_ID, d)
    t = np.concatenate([np.sort(rng.randint(1, CUT, e)), np.sort(rng.randint(CUT, 2 * CUT, d - e))])
    if d > e:
        t[e] = CUT  # the first ineligible entry sits exactly AT the cut: strictness decides
    return ids, t


def check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, k, salt, pick, shift=0):
    src, dst, pos, num = ops.sample_khop_temporal(g, t_et, dev(inp, shift), dev(cuts, shift), k, salt, pick)
    _, wsrc, wdst, wpos = ref.sample_layer(ip, ix, et, inp, cuts, k, salt, pick)
    m = int(num.item())
    assert m == wsrc.size
    np.testing.assert_array_equal(host_u32(pos, m), wpos)
    np.testing.assert_array_equal(host_u32(src, m), wsrc)
    np.testing.assert_array_equal(host_u32(dst, m), wdst)
    assert ops.device_status() == 0
    return host_u32(pos, m).copy()


def prefix_lengths(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, HUB})


@pytest.fixture(scope="module")
def prefix_graphs(ops):
    """Per fanout k: for every prefix length e a list that ends there (d = e) and one with 3000 ineligible entries behind
    it (d >> e; e = HUB: 300 behind), then three lists of HUB entries whose prefix is 3, k and 1025."""
    made = {}

    def get(k):
        if k not in made:
            rng = np.random.RandomState(k)
            lists, want_e = [], []
            for e in prefix_lengths(k):
                lists += [prefix_list(rng, e, e), prefix_list(rng, e, e + (3000 if e < HUB else 300))]
                want_e += [e, e]
            for e in (3, k, 1025):
                lists.append(prefix_list(rng, e, HUB))
                want_e.append(e)
            ip, ix, et = timed_graph(lists)
            for v, e in enumerate(want_e):
                assert ref.eligible(et[ip[v]:ip[v + 1]], CUT) == e
            made[k] = (ip, ix, et, ops.DeviceGraph(dev(ip), dev(ix)), dev(et))
        return made[k]
    yield get
    made.clear()


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
@pytest.mark.parametrize("k", [1, 10, 127])
def test_leaf_every_prefix_length(ops, prefix_graphs, k, pick):
    ip, ix, et, g, t_et = prefix_graphs(k)
    n = ip.size - 1
    inp = np.arange(n, dtype=np.uint32)
    cuts = np.full(n, CUT, np.uint32)
    for salt in (0, 0x4329F67E):
        check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, k, salt, pick)
    # the same lists without a cut: the tails are eligible too (other routes for the same lists)
    check_leaf(ops, g, t_et, ip, ix, et, inp, np.full(n, INF, np.uint32), k, 5, pick)


def cut_case_graph():
    """Node 0: 300 entries from 12 ids (every id at five times and more); positions 30 .. 99 share the time 500 (a tie
    that straddles the wave's lanes 63 | 64), the last two entries carry the time 0xffffffff.  Node 1: empty.  Node 2:
    one entry.  Node 3: 2000 entries, all at time 7."""
    rng = np.random.RandomState(3)
    t0 = np.concatenate([np.sort(rng.randint(10, 500, 30)), np.full(70, 500), np.sort(rng.randint(501, 900, 198)),
                         [INF, INF]]).astype(np.uint32)
    ids0 = rng.randint(0, 12, 300)
    assert min(np.bincount(ids0, minlength=12)) >= 5
    return timed_graph([(ids0, t0), ([], []), ([77], [40]), (rng.randint(0, NUM_ID, 2000), np.full(2000, 7))]), t0


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
def test_leaf_cuts_ties_and_duplicate_seeds(ops, pick):
    (ip, ix, et), t0 = cut_case_graph()
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    between = int(t0[120]) + 1 if t0[121] > t0[120] + 1 else int(t0[120])
    cuts0 = [0, int(t0[0]), int(t0[0]) + 1, 500, 501, between, 900, INF - 1, INF]
    # the same node again and again with another cut each time (duplicate seeds are independent), the others between
    inp = np.array([0] * len(cuts0) + [1, 2, 2, 2, 3, 3, 3, 0], np.uint32)
    cuts = np.array(cuts0 + [INF, 40, 41, 0, 7, 8, INF, 500], np.uint32)
    for k in (1, 10, 127):
        pos = check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, k, 0xC0FFEE + k, pick)
        assert (et[pos] < INF).all()  # a time of 2^32 - 1 is never eligible
    # strictness across the tie: with cut 500 none of the 70 entries AT 500 is eligible, with 501 all of them are
    assert ref.eligible(t0, 500) == 30 and ref.eligible(t0, 501) == 100


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
def test_leaf_misaligned_arrays(ops, pick):
    """indptr, indices, edge_time, the seeds and their cuts 4 bytes behind a 16-byte boundary (the 8-byte load of a
    list's bounds only needs 4-byte alignment)."""
    rng = np.random.RandomState(8)
    lists = [prefix_list(rng, e, e + t) for e, t in zip(rng.randint(0, 300, 400), rng.randint(0, 50, 400))]
    lists.append(prefix_list(rng, 1500, 1800))
    ip, ix, et = timed_graph(lists)
    g, t_et = ops.DeviceGraph(dev(ip, 1), dev(ix, 1)), dev(et, 1)
    inp = rng.permutation(401).astype(np.uint32)
    cuts = rng.choice([0, 300, CUT, CUT + 1, INF], 401).astype(np.uint32)
    check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, 10, 21, pick, shift=1)


@pytest.mark.parametrize("n", [0, 1, 4097])
def test_leaf_shapes_and_repeatability(ops, n):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(5000, mean_deg=30, seed=4)
    et = ref.sorted_times(ip, np.random.RandomState(4))
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    rng = np.random.RandomState(n)
    inp = rng.randint(0, 5000, n).astype(np.uint32)
    cuts = rng.randint(0, 1100, n).astype(np.uint32)
    if n == 0:
        z = torch.zeros(0, dtype=torch.int32, device="cuda")
        assert int(ops.sample_khop_temporal(g, t_et, z, z, 10, 1)[3].item()) == 0
        return
    a = check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, 10, 0x14D8859C, ref.UNIFORM)
    b = check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, 10, 0x14D8859C, ref.UNIFORM)
    assert np.array_equal(a, b)


def test_leaf_unsorted_list_stays_inside_the_list(ops):
    """A violated precondition: which edges come out is unspecified, but every position lies in its seed's list."""
    rng = np.random.RandomState(6)
    lists = [(rng.randint(0, NUM_ID, d), rng.randint(0, 2 * CUT, d)) for d in rng.randint(0, 1500, 300)]
    ip, ix, et = timed_graph(lists)
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    inp = np.arange(300, dtype=np.uint32)
    for pick in PICKS:
        src, dst, pos, num = ops.sample_khop_temporal(g, t_et, dev(inp), dev(np.full(300, CUT, np.uint32)), 10, 3, pick)
        m = int(num.item())
        s, p, d = host_u32(src, m).astype(np.int64), host_u32(pos, m).astype(np.int64), host_u32(dst, m)
        assert m <= 3000 and ((p >= ip[s]) & (p < ip[s + 1])).all() and (ix[p] == d).all()
    assert ops.device_status() == 0


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(3, request.param)  # GGMS_DEBUG_GRID_CAP
    yield request.param
    lib().ggms_debug_set_knob(3, -1)
    assert ops.device_status() == 0


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
def test_leaf_later_grid_rounds(ops, cap, pick):
    """3400 seeds under a grid cap of 1 and 3 workgroups: k_temporal_prefix takes 256 seeds per workgroup round,
    k_temporal_select 4 (a wave each, the next seed's prefix length carried over), k_temporal_hub one listed seed (14 of
    them: LDS reused behind the closing barrier)."""
    rng = np.random.RandomState(cap)
    deg = rng.randint(0, 120, 3400)
    hubs = rng.permutation(3400)[:14]
    deg[hubs] = rng.randint(1025, 3000, 14)
    lists = [prefix_list(rng, int(d), int(d) + int(x)) for d, x in zip(deg, rng.randint(0, 40, 3400))]
    ip, ix, et = timed_graph(lists)
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    inp = rng.permutation(3400).astype(np.uint32)
    cuts = rng.choice([CUT, CUT, CUT, 500, 0, INF], 3400).astype(np.uint32)
    check_leaf(ops, g, t_et, ip, ix, et, inp, cuts, 10, 0xABCD, pick)


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
def test_leaf_positions_past_2_31(ops, pick):
    """graphgen.high_offset_csr at 2^31: the hub's list has edge position 2^31 in its middle, half of the real nodes lie
    above it.  The reference works on the shifted graph (the filler at degree 0); its positions are shifted back."""
    from graphgen import high_offset_csr, high_offset_table
    g = high_offset_csr(1 << 31, seed=31)
    try:
        ip, ix = g.indptr_shifted, g.indices_shifted
        et = ref.sorted_times(ip, np.random.RandomState(31))
        graph = ops.DeviceGraph(dev(g.indptr), g.indices)
        t_et = high_offset_table(g, et)
        rng = np.random.RandomState(5)
        lo, hi = rng.permutation(g.below)[:150], rng.permutation(g.above)[:150]
        inp = np.concatenate([[g.hub, g.hub, g.hub], lo, hi]).astype(np.uint32)
        cuts = np.concatenate([[INF, 500, 3], rng.randint(0, 1100, 300)]).astype(np.uint32)
        for k in (5, 25):
            src, dst, pos, num = ops.sample_khop_temporal(graph, t_et, dev(inp), dev(cuts), k, 0xC0FFEE, pick)
            _, wsrc, wdst, wpos = ref.sample_layer(ip, ix, et, inp, cuts, k, 0xC0FFEE, pick)
            ea, fill = g.head.size, g.tail_start - g.head.size
            wpos = np.where(wpos >= ea, wpos.astype(np.int64) + fill, wpos).astype(np.uint32)
            m = int(num.item())
            assert m == wsrc.size and (wpos >= 1 << 31).any() and (wpos < 1 << 31).any()
            np.testing.assert_array_equal(host_u32(pos, m), wpos)
            np.testing.assert_array_equal(host_u32(src, m), wsrc)
            np.testing.assert_array_equal(host_u32(dst, m), wdst)
        assert ops.device_status() == 0
    finally:
        del g, graph, t_et
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_leaf_refuses_bad_arguments_on_the_device(ops):
    from xgnn_amd._lib import GgmsError
    ip, ix, et = timed_graph([prefix_list(np.random.RandomState(1), 5, 9)])
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    inp, cut = dev(np.zeros(4, np.uint32)), dev(np.full(4, CUT, np.uint32))
    for bad in (dict(fanout=0), dict(fanout=128), dict(pick=2)):
        kw = dict(fanout=5, pick=0)
        kw.update(bad)
        with pytest.raises(GgmsError, match="invalid argument"):
            ops.sample_khop_temporal(g, t_et, inp, cut, kw["fanout"], 1, kw["pick"])
    sharded = ops.DeviceGraph(None, None, part_indptr=[dev(ip), dev(ip)], part_indices=[dev(ix), dev(ix)], num_cache_node=1)
    with pytest.raises(GgmsError, match="invalid argument"):
        ops.sample_khop_temporal(sharded, t_et, inp, cut, 5, 1)
    assert ops.device_status() == 0


def test_link_seed_times(ops):
    rng = np.random.RandomState(2)
    et = rng.randint(0, 1 << 30, 5000).astype(np.uint32)
    for B, K in ((1, 1), (257, 3), (1000, 64)):
        eids = rng.randint(0, 5000, B).astype(np.uint32)
        eids[0] = 5000  # past the end: time 0, nothing is eligible
        want = np.where(eids < 5000, et[np.minimum(eids, 4999)], 0).astype(np.uint32)
        got = host_u32(ops.link_seed_times(dev(et), dev(eids), K))
        np.testing.assert_array_equal(got, np.concatenate([want, want, np.repeat(want, K)]))


# ---- the batch -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_graph(ops):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    et = ref.sorted_times(ip, np.random.RandomState(2))
    return ip, ix, et, ops.DeviceGraph(dev(ip), dev(ix)), dev(et)


def batch_seeds(rng, num_node=20_000):
    """301 seeds of which 40 are repeats with other times."""
    seeds = rng.permutation(num_node)[:301].astype(np.uint32)
    seeds[261:] = seeds[:40]
    times = rng.randint(0, 1100, 301).astype(np.uint32)
    times[5], times[6] = 0, INF
    assert (times[261:] != times[:40]).any()
    return seeds, times


def check_batch(bs, got, c, want, what=""):
    L = bs.L
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"], err_msg=what)
    np.testing.assert_array_equal(host_u32(got["node_cut"]), want["node_cut"], err_msg=what)
    assert c[COUNT_INPUT(L)] == want["input_nodes"].size and c[COUNT_STATUS(L)] == 0
    for i in range(L):
        gl, wl = got["layers"][i], want["layers"][i]
        assert (c[COUNT_EDGES(i)], c[COUNT_SRC(i)], c[COUNT_DST(i)]) == (wl["row"].size, wl["num_src"], wl["num_dst"]), (what, i)
        for key in ("row", "col", "eid"):
            np.testing.assert_array_equal(host_u32(gl[key]), wl[key], err_msg=f"{what} {key} layer {i}")
    np.testing.assert_array_equal(host_u32(bs.seed_ids()), want["seed_local"], err_msg=what)


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("fanouts", [[5], [5, 4], [3, 4, 5]], ids=["L1", "L2", "L3"])
def test_batch_equals_the_reference(ops, batch_graph, fanouts, direct, pick):
    ip, ix, et, g, t_et = batch_graph
    bs = ops.TemporalBatchSampler(g, t_et, fanouts, 301, pick=pick, direct_table=direct, max_seeds=301)
    rng = np.random.RandomState(len(fanouts))
    for rep in range(2):  # the second batch finds the first one's words in both tables
        seeds, times = batch_seeds(rng)
        salt = labor.batch_salt(42, rep, 17)
        bs.sample(dev(seeds), dev(times), salt)
        got = bs.result()
        want = ref.sample_batch(ip, ix, et, seeds, times, fanouts, salt, pick)
        check_batch(bs, got, bs.counts.cpu().tolist(), want, f"rep {rep}")
        check_no_leak(want, et, seeds, times)


def test_two_batches_on_one_cut_table_and_the_stamp_wrap(ops, batch_graph):
    """Stamps 1 and 2: the second batch has the first one's seeds with LARGER times, so a stale word read as live would
    show as a cut that is too small.  Then stamp 0xffffffff, and after it the table zeroed and stamp 1 again."""
    ip, ix, et, g, t_et = batch_graph
    fanouts = [5, 4]
    bs = ops.TemporalBatchSampler(g, t_et, fanouts, 301, max_seeds=301)
    rng = np.random.RandomState(77)
    seeds, times = batch_seeds(rng)
    times = np.minimum(times, 400).astype(np.uint32)
    plan = [(1, times), (2, times + 500), (0xFFFFFFFF, times + 100), (None, times + 300)]
    for stamp, t in plan:
        bs.sample(dev(seeds), dev(t), 9, stamp=stamp)
        if stamp is None:
            assert bs.stamp == 1  # wrapped: the sampler zeroed its table
        want = ref.sample_batch(ip, ix, et, seeds, t, fanouts, 9)
        check_batch(bs, bs.result(), bs.counts.cpu().tolist(), want, f"stamp {stamp}")


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_batch_without_cuts_equals_the_khop_labor_batch(ops, batch_graph, direct):
    """All cuts 0xffffffff (and no edge at that time): ggms_sample_batch(GGMS_KHOP_LABOR) on the same graph, the
    project's existing kernels, gives the same batch."""
    ip, ix, et, g, t_et = batch_graph
    fanouts = [3, 4, 5]
    seeds = np.random.RandomState(3).permutation(20_000)[:301].astype(np.uint32)
    seeds[300] = seeds[0]
    tb = ops.TemporalBatchSampler(g, t_et, fanouts, 301, direct_table=direct, max_seeds=301)
    lb = ops.BatchSampler(g, fanouts, 301, sample_type=ops.KHOP_LABOR, direct_table=direct)
    tb.sample(dev(seeds), dev(np.full(301, INF, np.uint32)), 0xDA2897D6)
    lb.sample(dev(seeds), labor_salt=0xDA2897D6)
    a, b = tb.result(), lb.result()
    np.testing.assert_array_equal(host_u32(a["input_nodes"]), host_u32(b["input_nodes"]))
    assert tb.counts.cpu().tolist() == lb.counts.cpu().tolist()
    for la, lb_ in zip(a["layers"], b["layers"]):
        np.testing.assert_array_equal(host_u32(la["row"]), host_u32(lb_["row"]))
        np.testing.assert_array_equal(host_u32(la["col"]), host_u32(lb_["col"]))
    assert (host_u32(a["node_cut"]) == INF).all()
    # the positions are those of the edges: indices[eid] is the row's node, and it lies in the col's list
    nodes = host_u32(a["input_nodes"]).astype(np.int64)
    for la in a["layers"]:
        eid, row, col = (host_u32(la[key]).astype(np.int64) for key in ("eid", "row", "col"))
        assert (ix[eid] == nodes[row]).all() and (eid >= ip[nodes[col]]).all() and (eid < ip[nodes[col] + 1]).all()


@pytest.mark.parametrize("pick", PICKS, ids=pick_ids)
def test_batch_never_leaks_on_a_clustered_graph(ops, pick):
    """20 000-node community graph (neighbourhoods overlap heavily: many nodes are reached under several times), random
    times: the GPU batch equals the reference, and the reference's snapshots satisfy check_no_leak."""
    ip, ix = labor.community_graph()
    et = ref.sorted_times(ip, np.random.RandomState(1), 1, 5000)
    g, t_et = ops.DeviceGraph(dev(ip), dev(ix)), dev(et)
    rng = np.random.RandomState(4)
    seeds = rng.randint(0, 2000, 400).astype(np.uint32)  # four communities: repeats and shared neighbours
    times = rng.randint(0, 5500, 400).astype(np.uint32)
    fanouts = [5, 4]
    bs = ops.TemporalBatchSampler(g, t_et, fanouts, 400, pick=pick, max_seeds=400)
    bs.sample(dev(seeds), dev(times), 123)
    got = bs.result()
    want = ref.sample_batch(ip, ix, et, seeds, times, fanouts, 123, pick)
    check_batch(bs, got, bs.counts.cpu().tolist(), want)
    check_no_leak(want, et, seeds, times)
    # and directly on the GPU's own output: every edge lies before the smallest root time its col can serve, which
    # the final cut of the col bounds from below only -- so the direct statement uses the seeds: a first-layer edge lies
    # before the time of every raw seed that is its col
    first = got["layers"][len(fanouts) - 1]
    eid, col = host_u32(first["eid"]).astype(np.int64), host_u32(first["col"]).astype(np.int64)
    root_time = np.full(host_u32(got["input_nodes"]).size, INF, np.int64)
    np.minimum.at(root_time, want["seed_local"], times.astype(np.int64))
    assert (et[eid] < root_time[col]).all()
