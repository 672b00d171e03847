"""khop_labor on the GPU against its numpy statement (tests/khop_labor_ref.py), bit for bit: the leaf over every list
length at which the kernel changes route, hubs (a plain one and two that defeat the pre-filter), ties, shapes, sharded
views, the batch chain on both table layouts, and the claim the sampler exists for -- fewer input nodes than khop0."""
import numpy as np
import pytest

import khop_labor_ref as ref
from xgnn_amd._lib import COUNT_EDGES, COUNT_INPUT, COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# where xgnn_amd/csrc/sample_labor.hip changes route (d = list length, k = fanout):
#   d <= k                    the list is copied
#   d <= kLaborWave1   = 64   one wave, 1 key per lane
#   d <= kLaborWave4   = 256  one wave, 4 keys per lane
#   d <= kLaborWaveMax = 1024 one wave, 16 keys per lane
#   beyond                    one workgroup: pre-filter ((2 k + 64) / d of the hash range into kLaborCand = 1024 LDS
#                             slots), the exact route when it keeps fewer than k or more than 1024
WAVE1, WAVE4, WAVE_MAX, CAND = 64, 256, 1024, 1024
NUM_ID = 1 << 20  # neighbour ids of the leaf graphs (a leaf never follows them)


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


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


def graph_of_lists(lists):
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum([len(x) for x in lists])
    ix = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if ip[-1] else np.zeros(0, np.uint32)
    return ip, ix


def check_leaf(ops, g, ip, ix, inp, k, salt):
    t_in = dev(inp) if inp.size else torch.zeros(0, dtype=torch.int32, device="cuda")
    src, dst, num = ops.sample_khop_labor(g, t_in, k, salt)
    _, wsrc, wdst = ref.sample_layer(ip, ix, inp, k, salt)
    m = int(num.item())
    assert m == wsrc.size
    np.testing.assert_array_equal(host_u32(src, m), wsrc)
    np.testing.assert_array_equal(host_u32(dst, m), wdst)
    assert ops.device_status() == 0
    return host_u32(src, m).copy(), host_u32(dst, m).copy()


@pytest.mark.parametrize("k", [1, 5, 25, 127])
def test_leaf_every_list_length(ops, k):
    D = sorted({0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025,
                WAVE1 - 1, WAVE1, WAVE1 + 1, WAVE4 - 1, WAVE4, WAVE4 + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1,
                2 * k + 64, 3000})
    rng = np.random.RandomState(k)
    lists = [rng.randint(0, NUM_ID, d) for d in D]
    ip, ix = graph_of_lists(lists)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    for salt in (0, 0x4329F67E):
        check_leaf(ops, g, ip, ix, np.arange(len(D), dtype=np.uint32), k, salt)


def _ids_with_hash(salt, lo, hi, count, rng):
    """`count` ids (with repeats where too few exist) whose fmix32(id ^ salt) lies in [lo, hi)."""
    ids = np.arange(1 << 23, dtype=np.uint64)
    h = ref.fmix32(ids ^ np.uint64(salt))
    pool = ids[(h >= lo) & (h < hi)].astype(np.uint32)
    assert pool.size >= 256
    return pool[rng.randint(0, pool.size, count)] if pool.size < count else rng.permutation(pool)[:count]


@pytest.fixture(scope="module")
def hub_graph(ops):
    """300 ordinary lists, then three lists of 100 000: a plain hub, one whose every hash is >= 0xC0000000 (the
    pre-filter keeps nothing) and one whose every hash is < 0x00100000 (it keeps everything, ties included)."""
    salt = 0x0C6EC80C
    rng = np.random.RandomState(11)
    lists = [rng.randint(0, NUM_ID, d) for d in rng.randint(0, 120, 300)]
    lists.append(rng.randint(0, NUM_ID, 100_000))
    lists.append(_ids_with_hash(salt, 0xC0000000, 1 << 32, 100_000, rng))
    lists.append(_ids_with_hash(salt, 0, 0x00100000, 100_000, rng))
    ip, ix = graph_of_lists(lists)
    h = ref.fmix32(ix[ip[301]:ip[303]].astype(np.uint64) ^ np.uint64(salt))
    assert h[:100_000].min() >= 0xC0000000 and h[100_000:].max() < 0x00100000
    return salt, ip, ix, ops.DeviceGraph(dev(ip), dev(ix))


@pytest.mark.parametrize("k", [1, 5, 127])
@pytest.mark.parametrize("hub", [300, 301, 302], ids=["plain", "prefilter-too-few", "prefilter-too-many"])
def test_leaf_hub_among_ordinary_seeds(ops, hub_graph, hub, k):
    salt, ip, ix, g = hub_graph
    inp = np.concatenate([np.arange(150), [hub], np.arange(150, 300)]).astype(np.uint32)
    check_leaf(ops, g, ip, ix, inp, k, salt)


def test_leaf_ties_break_by_position(ops):
    rng = np.random.RandomState(5)
    lists = [np.concatenate([rng.randint(0, NUM_ID, 30), np.full(200, 777), rng.randint(0, NUM_ID, 20)]),
             np.full(200, 777), np.concatenate([np.full(1500, 31), rng.randint(0, NUM_ID, 100)])]
    ip, ix = graph_of_lists(lists)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    picked_run = 0
    for salt in range(40):
        _, dst = check_leaf(ops, g, ip, ix, np.arange(3, dtype=np.uint32), 5, salt)
        picked_run += int((dst[:5] == 777).sum() > 0)
    assert picked_run > 0  # the run of equal ids was selected from at least once (its first positions: the reference)


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
def test_leaf_shapes_duplicates_and_repeatability(ops, n):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(5000, mean_deg=30, seed=4)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    inp = np.random.RandomState(n).randint(0, 5000, n).astype(np.uint32)
    if n > 1:
        inp[n // 2] = inp[0]  # a duplicated seed is sampled independently: same neighbours
    a = check_leaf(ops, g, ip, ix, inp, 10, 0x14D8859C)
    b = check_leaf(ops, g, ip, ix, inp, 10, 0x14D8859C)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("P", [2, 3, 8])
def test_leaf_through_sharded_views(ops, P):
    """Nodes below num_cache_node in P shards, the rest in the whole CSR of slot P: equal to the unsharded call."""
    import oracle
    from graphgen import hub_csr
    ip, ix = hub_csr(3000, num_hub=6, hub_deg=6000, seed=P)
    ncn = 1800
    parts = [oracle.partition_graph(ip, ix, r, P, ncn) for r in range(P)]
    g = ops.DeviceGraph(None, None, part_indptr=[dev(p[0]) for p in parts] + [dev(ip)],
                        part_indices=[dev(p[1]) for p in parts] + [dev(ix)], num_cache_node=ncn)
    plain = ops.DeviceGraph(dev(ip), dev(ix))
    inp = np.random.RandomState(P).permutation(3000)[:700].astype(np.uint32)
    for k in (5, 25):
        a = check_leaf(ops, g, ip, ix, inp, k, 99)
        b = check_leaf(ops, plain, ip, ix, inp, k, 99)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def run_batch(ops, bs, seeds, salt, distinct):
    bs.sample(dev(seeds), distinct=distinct, labor_salt=salt)
    c = bs.counts.cpu().tolist()
    assert c[COUNT_STATUS(bs.L)] == 0  # the batch's status word
    return bs.result(), c


@pytest.fixture(scope="module")
def batch_graph(ops):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    return ip, ix, ops.DeviceGraph(dev(ip), dev(ix))


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("fanouts", [[10], [10, 25], [15, 10, 5]], ids=["L1", "L2", "L3"])
def test_batch_equals_the_reference_chain(ops, batch_graph, fanouts, direct):
    ip, ix, g = batch_graph
    bs = ops.BatchSampler(g, fanouts, 300, sample_type=ops.KHOP_LABOR, direct_table=direct)
    assert bs.states is None
    rng = np.random.RandomState(len(fanouts))
    for rep, distinct in enumerate([False, True, False]):
        seeds = rng.permutation(20_000)[:300].astype(np.uint32)
        if rep == 2:
            seeds[5] = seeds[0]  # a duplicated seed: local ids of raw seeds go through the table
        salt = ref.batch_salt(42, rep, 17)
        got, c = run_batch(ops, bs, seeds, salt, distinct)
        want = ref.sample_batch(ip, ix, seeds, fanouts, salt)
        np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"])
        assert c[COUNT_INPUT(len(fanouts))] == want["input_nodes"].size
        for i in range(len(fanouts)):
            gl, wl = got["layers"][i], want["layers"][i]
            assert (c[COUNT_EDGES(i)], gl["num_src"], gl["num_dst"]) == (wl["row"].size, wl["num_src"], wl["num_dst"]), (rep, i)
            np.testing.assert_array_equal(host_u32(gl["row"]), wl["row"], err_msg=f"row layer {i} rep {rep}")
            np.testing.assert_array_equal(host_u32(gl["col"]), wl["col"], err_msg=f"col layer {i} rep {rep}")


def test_fewer_input_nodes_than_independent_sampling(ops):
    """256 distinct seeds, fanouts [10, 10] on the community graph: khop_labor's batch has at most 0.85 x the input
    nodes of khop0's (numpy restatement: 0.74 - 0.75)."""
    ip, ix = ref.community_graph()
    g = ops.DeviceGraph(dev(ip), dev(ix))
    seeds = np.random.RandomState(1).permutation(ip.size - 1)[:256].astype(np.uint32)
    nodes = {}
    for name, code in (("khop0", ops.KHOP0), ("khop_labor", ops.KHOP_LABOR)):
        bs = ops.BatchSampler(g, [10, 10], 256, sample_type=code, seed=3)
        got, _ = run_batch(ops, bs, seeds, 0xDA2897D6, True)
        nodes[name] = got["input_nodes"].numel()
        edges = [l["row"].numel() for l in got["layers"]]
        print(f"{name}: input nodes {nodes[name]}, edges {edges}")
    print(f"ratio {nodes['khop_labor'] / nodes['khop0']:.3f}")
    assert nodes["khop_labor"] <= 0.85 * nodes["khop0"]
