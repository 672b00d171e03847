"""khop_typed_temporal on the GPU against its numpy statement (tests/khop_typed_temporal_ref.py), bit for bit.  The leaf:
every eligible-prefix length at which the kernels change route, as the first, a middle and the last segment, with a
repeated time on both sides of the cut; zero fanouts, an absent relation, cut 0, duplicate seeds with different cuts;
R = 1 / 2 / 5 / 32; misaligned arrays; later grid rounds; an unsorted list; the two identities.  The batch: both table
layouts, a fanout row per layer, repeated seeds with different times."""
import numpy as np
import pytest

import khop_labor_ref as labor
import khop_typed_ref as typed
import khop_typed_temporal_ref as ref
from xgnn_amd._lib import COUNT_DST, COUNT_EDGES, COUNT_INPUT, COUNT_SRC, COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HUB, CUT = 40_000, 5000
PICKS = [ref.UNIFORM, ref.RECENT]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a, shift=0):
    """The array on the device; `shift` elements behind a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    if shift:
        buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
        buf[shift:shift + t.numel()] = t
        t = buf[shift:shift + t.numel()]
        assert t.data_ptr() % 16 == shift * t.element_size()
    return t


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


class Graph:
    def __init__(self, ops, ip, ix, et, tm, shift=(0, 0, 0)):
        self.ip, self.ix, self.et, self.tm = ip, ix, et, tm
        self.g = ops.DeviceGraph(dev(ip, shift[0]), dev(ix, shift[0]))
        self.d_et, self.d_tm = dev(et, shift[1]), dev(tm, shift[2])


def check_leaf(ops, G, inp, cuts, tf, salt, pick, shift=0):
    got = ops.sample_khop_typed_temporal(G.g, G.d_et, G.d_tm, tf, dev(inp, shift), dev(cuts, shift), salt, pick)
    _, *want = ref.sample_layer(G.ip, G.ix, G.et, G.tm, inp, cuts, tf, salt, pick)
    m = int(got[4].item())
    assert m == want[0].size
    for g, w, name in zip((got[2], got[3], got[0], got[1]), (want[2], want[3], want[0], want[1]), ("pos", "type", "src", "dst")):
        np.testing.assert_array_equal(g.cpu().numpy()[:m].view(w.dtype), w, err_msg=name)
    assert ops.device_status() == 0


def segment_times(n, e):
    """n times of which the first e lie before CUT: the last two of them repeat CUT - 1, the first three behind repeat CUT."""
    before = np.minimum(np.arange(e) + CUT - 1 - max(e - 2, 0), CUT - 1) if e <= CUT else np.minimum(np.arange(e) // 16, CUT - 1)
    return np.concatenate([before, CUT + np.maximum(np.arange(n - e) - 2, 0)]).astype(np.uint32)


@pytest.fixture(scope="module")
def prefix_graphs(ops):
    """Per fanout k, three relations: for every e a list whose first / middle / last segment has e entries before CUT and
    7 behind (the others: 2 of 5 and 1 of 3), then a HUB-entry list whose eligible prefixes have 3, 7 and 0 entries."""
    made = {}

    def get(k):
        if k not in made:
            lists = []
            for e in sorted({0, 1, k, k + 1, 64, 65, 256, 257, 1024, 1025, HUB}):
                lists += [[(e + 7, e), (5, 2), (3, 1)], [(3, 1), (e + 7, e), (5, 2)], [(5, 2), (3, 1), (e + 7, e)]]
            lists.append([(HUB // 2, 3), (HUB // 2 - 9, 7), (9, 0)])
            ip, ix, et = typed.segment_graph([[n for n, _ in li] for li in lists])
            tm = np.concatenate([segment_times(n, e) for li in lists for n, e in li])
            made[k] = Graph(ops, ip, ix, et, tm)
        return made[k]
    yield get
    made.clear()


@pytest.mark.parametrize("pick", PICKS, ids=["uniform", "recent"])
@pytest.mark.parametrize("k", [1, 10, 127])
def test_leaf_every_prefix_length(ops, prefix_graphs, k, pick):
    G = prefix_graphs(k)
    inp = np.arange(G.ip.size - 1, dtype=np.uint32)
    cuts = np.full(inp.size, CUT, np.uint32)
    check_leaf(ops, G, inp, cuts, [k, k, k], 0x4329F67E, pick)
    check_leaf(ops, G, inp, cuts, [k, 0, k, 5], 7, pick)  # a zero fanout, and R = 4: a relation that no list holds
    # cut 0, a cut before everything, behind everything, "no cut"; the same seeds again under other cuts
    other = np.resize(np.array([0, 1, CUT - 1, CUT + 1, 1 << 30, ref.INF], np.uint32), inp.size)
    check_leaf(ops, G, np.concatenate([inp, inp]), np.concatenate([other, cuts]), [k, 3, k], 5, pick)


def random_graph(ops, rng, n, R, max_deg=300, hubs=3, hub_deg=(1100, 3000), shift=(0, 0, 0)):
    """Random (type, time)-sorted lists (some empty, `hubs` long ones, every tenth all one relation), one relation absent."""
    deg = rng.randint(0, max_deg, n)
    deg[rng.randint(0, n, max(1, n // 40))] = 0
    deg[rng.permutation(n)[:hubs]] = rng.randint(hub_deg[0], hub_deg[1], hubs)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = rng.randint(0, n, int(ip[-1])).astype(np.uint32)
    w = rng.random_sample(R) + 0.05
    if R > 1:
        w[(R // 2 + 1) % R] = 0
    et = typed.sorted_types(ip, rng, R, w / w.sum())
    for v in range(0, n, 10):
        et[ip[v]:ip[v + 1]] = et[ip[v]] if ip[v] < ip[v + 1] else 0
    return Graph(ops, ip, ix, et, ref.sorted_times(ip, et, rng), shift)


def random_cuts(rng, n):
    cuts = rng.randint(0, 1100, n).astype(np.uint32)
    cuts[::7], cuts[3::11] = ref.INF, 0
    return cuts


@pytest.mark.parametrize("pick", PICKS, ids=["uniform", "recent"])
@pytest.mark.parametrize("R", [1, 2, 5, 32])
def test_leaf_relation_counts_and_identities(ops, R, pick):
    rng = np.random.RandomState(R)
    G = random_graph(ops, rng, 600, R)
    inp = rng.randint(0, 600, 700).astype(np.uint32)
    inp[650:] = inp[:50]  # duplicate seeds, other cuts
    cuts = random_cuts(rng, 700)
    tf = rng.randint(0, 6, R)
    tf[0], tf[-1] = (127 if R > 1 else 10), max(tf[-1], 1)
    check_leaf(ops, G, inp, cuts, tf.tolist(), 0xC0FFEE + R, pick)
    if R == 1:  # bit for bit khop_temporal with fanout k_0
        a = ops.sample_khop_typed_temporal(G.g, G.d_et, G.d_tm, tf.tolist(), dev(inp), dev(cuts), 9, pick)
        b = ops.sample_khop_temporal(G.g, G.d_tm, dev(inp), dev(cuts), int(tf[0]), 9, pick)
        m = int(b[3].item())
        assert m == int(a[4].item()) and all(torch.equal(a[j][:m], b[j][:m]) for j in range(3))
    if pick == ref.UNIFORM:  # every cut = "no cut": bit for bit khop_typed
        a = ops.sample_khop_typed_temporal(G.g, G.d_et, G.d_tm, tf.tolist(), dev(inp), dev(np.full(700, ref.INF, np.uint32)), 9)
        b = ops.sample_khop_typed(G.g, G.d_et, tf.tolist(), dev(inp), 9)
        m = int(b[4].item())
        assert m == int(a[4].item()) and all(torch.equal(a[j][:m], b[j][:m]) for j in range(4))


@pytest.mark.parametrize("shift", [1, 3])
def test_leaf_misaligned_arrays(ops, shift):
    """edge_type 1 and 3 bytes behind a 16-byte boundary; indptr, indices, the times, the seeds and the cuts 4 bytes."""
    rng = np.random.RandomState(8 + shift)
    G = random_graph(ops, rng, 400, 5, shift=(1, shift, 1))
    check_leaf(ops, G, rng.permutation(400).astype(np.uint32), random_cuts(rng, 400), [3, 0, 10, 1, 127], 21, ref.UNIFORM, shift=1)


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(3, request.param)  # GGMS_DEBUG_GRID_CAP
    yield request.param
    lib().ggms_debug_set_knob(3, -1)


@pytest.mark.parametrize("R", [1, 5])
def test_leaf_later_grid_rounds(ops, cap, R):
    """3401 seeds under a grid cap of 1 and 3 workgroups: k_tt_bounds takes 256 / G seeds per workgroup round, k_tt_select
    4, k_tt_hub one listed seed (14 hubs whose prefixes before 900 are mostly above 1024 entries)."""
    rng = np.random.RandomState(cap)
    G = random_graph(ops, rng, 3401, R, max_deg=120, hubs=14, hub_deg=(6000, 9000))
    cuts = np.where(rng.randint(0, 4, 3401) == 0, ref.INF, 900).astype(np.uint32)
    check_leaf(ops, G, rng.permutation(3401).astype(np.uint32), cuts, [10] if R == 1 else [4, 2, 2, 1, 3], 0xABCD, ref.UNIFORM)


@pytest.mark.parametrize("pick", PICKS, ids=["uniform", "recent"])
def test_leaf_unsorted_list_stays_inside_the_list(ops, pick):
    """A violated precondition (and types >= R): which edges come out is unspecified, but every position lies in its
    seed's list, no seed emits more than K edges, and the run completes with a clean status."""
    rng = np.random.RandomState(6)
    ip = np.concatenate([[0], np.cumsum(rng.randint(0, 1500, 300))]).astype(np.uint32)
    E = int(ip[-1])
    G = Graph(ops, ip, rng.randint(0, 1 << 20, E).astype(np.uint32), rng.randint(0, 7, E).astype(np.uint8),
              rng.randint(0, 1000, E).astype(np.uint32))
    tf = [3, 0, 10, 1, 4]
    src, dst, pos, typ, num = ops.sample_khop_typed_temporal(G.g, G.d_et, G.d_tm, tf, dev(np.arange(300, dtype=np.uint32)),
                                                             dev(random_cuts(rng, 300)), 3, pick)
    m = int(num.item())
    s, p, d = host_u32(src, m).astype(np.int64), host_u32(pos, m).astype(np.int64), host_u32(dst, m)
    assert m <= 300 * sum(tf) and ((p >= ip[s]) & (p < ip[s + 1])).all() and (G.ix[p] == d).all()
    assert (np.diff(s) >= 0).all() and np.bincount(s, minlength=300).max() <= sum(tf)
    assert ops.device_status() == 0


# ---- the batch -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_graph(ops):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    rng = np.random.RandomState(2)
    et = typed.sorted_types(ip, rng, 4, [0.6, 0.0, 0.37, 0.03])  # relation 1 absent, relation 3 rare
    return Graph(ops, ip, ix, et, ref.sorted_times(ip, et, rng))


@pytest.mark.parametrize("pick", PICKS, ids=["uniform", "recent"])
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_batch_equals_the_reference(ops, batch_graph, direct, pick):
    G = batch_graph
    tfs = [[3, 2, 0, 2], [0, 1, 4, 1]]  # another row of fanouts for every layer
    bs = ops.TypedTemporalBatchSampler(G.g, G.d_et, G.d_tm, tfs, 301, pick=pick, direct_table=direct, max_seeds=301)
    rng = np.random.RandomState(5)
    lowered = 0
    for rep in range(2):  # the second batch finds the first one's words in the tables
        seeds = rng.permutation(20_000)[:301].astype(np.uint32)
        seeds[261:] = seeds[:40]  # repeated seeds, other times
        times = rng.randint(1, 1100, 301).astype(np.uint32)
        salt = labor.batch_salt(42, rep, 17)
        bs.sample(dev(seeds), dev(times), salt)
        got, c = bs.result(), bs.counts.cpu().tolist()
        want = ref.sample_batch(G.ip, G.ix, G.et, G.tm, seeds, times, tfs, salt, pick)
        np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"])
        np.testing.assert_array_equal(host_u32(got["node_cut"]), want["node_cut"])
        np.testing.assert_array_equal(host_u32(bs.seed_ids()), want["seed_local"])
        assert c[COUNT_INPUT(2)] == want["input_nodes"].size and c[COUNT_STATUS(2)] == 0
        for i, (gl, wl) in enumerate(zip(got["layers"], want["layers"])):
            assert (c[COUNT_EDGES(i)], c[COUNT_SRC(i)], c[COUNT_DST(i)]) == (wl["row"].size, wl["num_src"], wl["num_dst"])
            for key in ("row", "col", "eid"):
                np.testing.assert_array_equal(host_u32(gl[key]), wl[key], err_msg=f"rep {rep} {key} layer {i}")
            np.testing.assert_array_equal(gl["etype"].cpu().numpy(), wl["etype"], err_msg=f"rep {rep} etype layer {i}")
        # a node reached under two times is sampled before the smaller: layer 0's edges lie before their seed's cut as
        # the layer found it, which for some nodes is below the time they first came with
        l0 = want["layers"][0]
        assert (G.tm[host_u32(got["layers"][0]["eid"]).astype(np.int64)] < l0["cut_at_start"][l0["col"]]).all()
        first = {}
        for v, t in zip(seeds.tolist(), times.tolist()):
            first.setdefault(v, t)
        lowered += sum(want["node_cut"][j] < first[v] for j, v in enumerate(want["input_nodes"].tolist()) if v in first)
    assert lowered > 0
