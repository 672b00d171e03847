"""khop_labor_weighted on the GPU against its numpy statement (tests/khop_labor_weighted_ref.py), bit for bit: the leaf
at every list length where xgnn_amd/csrc/sample_labor_weighted.hip changes route (copy d <= k; one wave with 1 / 4 / 16
pairs per lane up to 64 / 256 / 1024; a workgroup beyond), hubs that take each of the hub kernel's routes, the clamp,
the marginals against the analytic law, the batch chain on both table layouts, and later grid-stride rounds."""
import numpy as np
import pytest

import khop_labor_weighted_ref as ref
from xgnn_amd._lib import COUNT_EDGES, COUNT_INPUT, COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NUM_ID = 1 << 20  # neighbour ids of the leaf graphs (a leaf never follows them)
GRID_CAP = 3      # GGMS_DEBUG_GRID_CAP


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


def graph_of_lists(lists):
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum([len(x) for x in lists])
    return ip, np.concatenate([np.asarray(x, np.uint32) for x in lists])


def log_uniform(rng, n):
    return np.exp2(rng.uniform(-8, 8, n)).astype(np.float32)


def check_leaf(ops, g, ew_dev, ip, ix, ew, inp, k, salt):
    src, dst, pos, num = ops.sample_khop_labor_weighted(g, ew_dev, dev(inp), k, salt)
    _, wsrc, wdst, wpos = ref.sample_layer(ip, ix, ew, inp, k, salt)
    m = int(num.item())
    assert m == wsrc.size
    np.testing.assert_array_equal(host_u32(pos, m), wpos)
    np.testing.assert_array_equal(host_u32(src, m), wsrc)
    np.testing.assert_array_equal(host_u32(dst, m), wdst)
    assert ops.device_status() == 0


def boundary_graph(ops, k):
    D = sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2 * k + 64, 3000})
    rng = np.random.RandomState(k)
    ip, ix = graph_of_lists([rng.randint(0, NUM_ID, d) for d in D])
    ew = log_uniform(rng, ix.size)
    return ip, ix, ew, ops.DeviceGraph(dev(ip), dev(ix)), dev(ew), len(D)


@pytest.mark.parametrize("k", [1, 25, 127])
def test_leaf_at_the_route_boundaries(ops, k):
    ip, ix, ew, g, ew_dev, n = boundary_graph(ops, k)
    for salt in (0, 0x4329F67E):
        check_leaf(ops, g, ew_dev, ip, ix, ew, np.arange(n, dtype=np.uint32), k, salt)


@pytest.mark.parametrize("cap", [1, 3])
def test_leaf_later_grid_rounds(ops, cap):
    """3400 seeds under a grid cap of 1 and 3 workgroups: the wave kernel's prefetch hand-over over many rounds, the hub
    kernel's LDS reused from list to list."""
    from xgnn_amd import lib
    ip, ix, ew, g, ew_dev, n = boundary_graph(ops, 25)
    inp = np.random.RandomState(cap).randint(0, n, 3400).astype(np.uint32)
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        check_leaf(ops, g, ew_dev, ip, ix, ew, inp, 25, 0x51ED270B)
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


HUB_SALT, HUB_K, HUB_D = 0x0C6EC80C, 25, 100_000


@pytest.fixture(scope="module")
def hub_graph(ops):
    """20 ordinary lists, then four lists of 100 000: plain weights (pre-filter route); three weights of 2^30 among 2^-10
    (they carry W: fewer than k survivors); one id with equal weights whose variate lies under the threshold (every key
    ties and survives: the buffer overflows); out-of-range weights mixed in (the clamp)."""
    rng = np.random.RandomState(11)
    lists = [rng.randint(0, NUM_ID, d) for d in rng.randint(0, 120, 20)] + [rng.randint(0, NUM_ID, HUB_D) for _ in range(2)]
    ids = np.arange(1 << 16, dtype=np.uint64)
    lists.append(np.full(HUB_D, ids[np.argmax(ref.labor.fmix32(ids ^ np.uint64(HUB_SALT)))]))  # the smallest E of 65536
    lists.append(rng.randint(0, NUM_ID, HUB_D))
    ip, ix = graph_of_lists(lists)
    ew = log_uniform(rng, ix.size)
    ew[ip[21]:ip[22]] = 2.0 ** -10
    ew[ip[21] + np.array([5, 40_000, 99_999])] = 2.0 ** 30
    ew[ip[22]:ip[23]] = 3.0
    ew[ip[23]:ip[24]:7] = np.resize(np.array([0, -1, np.inf, np.nan, -np.inf, 2.0 ** 60, 1e-30], np.float32), len(range(0, HUB_D, 7)))
    return ip, ix, ew, ops.DeviceGraph(dev(ip), dev(ix)), dev(ew)


@pytest.mark.parametrize("hub", [20, 21, 22, 23], ids=["plain", "skewed", "ties-overflow", "clamp"])
def test_leaf_hub(ops, hub_graph, hub):
    ip, ix, ew, g, ew_dev = hub_graph
    inp = np.concatenate([np.arange(10), [hub], np.arange(10, 20)]).astype(np.uint32)
    check_leaf(ops, g, ew_dev, ip, ix, ew, inp, HUB_K, HUB_SALT)


def test_leaf_clamp_decides_the_selection(ops):
    """Lists of 26 .. 900 entries (every wave route) in which seven of ten weights are 0, negative, -inf, NaN or below 2^-40:
    with k = 25 most edges selected from the short lists carry one of them, and their order is that of E / 2^-40 -- unclamped, their keys would
    be inf, NaN or negative bit patterns and tie or order otherwise."""
    rng = np.random.RandomState(6)
    ip, ix = graph_of_lists([rng.randint(0, NUM_ID, d) for d in (26, 40, 64, 200, 900)])
    ew = np.resize(np.array([0, -1, 1.0, -np.inf, np.nan, 1e-30, -0.0, 2.0 ** -41, np.inf, 2.0 ** -39], np.float32), ix.size)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    for salt in (1, 0x7F4A7C15):
        check_leaf(ops, g, dev(ew), ip, ix, ew, np.arange(5, dtype=np.uint32), 25, salt)


def test_marginals_follow_the_weights(ops):
    """20 000 seeds, each with 8 distinct random neighbours weighted 1, 2, 4 .. 128, fanout 1: position i is drawn
    with probability w_i / 255; every frequency within 5 binomial standard deviations."""
    n = 20_000
    rng = np.random.RandomState(3)
    ix = (rng.randint(0, 1 << 28, n)[:, None] * 8 + np.argsort(rng.rand(n, 8), axis=1)).astype(np.uint32).ravel()
    ip = (np.arange(n + 1) * 8).astype(np.uint32)
    ew = np.tile(np.exp2(np.arange(8)).astype(np.float32), n)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    _, _, pos, num = ops.sample_khop_labor_weighted(g, dev(ew), dev(np.arange(n, dtype=np.uint32)), 1, 0x2545F491)
    assert int(num.item()) == n
    freq = np.bincount(host_u32(pos, n) % 8, minlength=8) / n
    p = np.exp2(np.arange(8)) / 255
    print("frequencies", freq, "law", p)
    assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n))


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_batch_equals_the_reference_chain(ops, direct):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(3000, mean_deg=30, seed=2)
    ew = log_uniform(np.random.RandomState(8), ix.size)
    fanouts = [5, 10]
    bs = ops.LaborWeightedBatchSampler(ops.DeviceGraph(dev(ip), dev(ix)), dev(ew), fanouts, 1000, direct_table=direct)
    seeds = np.random.RandomState(1).randint(0, 3000, 1000).astype(np.uint32)  # with repeats
    bs.sample(dev(seeds), salt=0x3C6EF372)
    got, c = bs.result(), bs.counts.cpu().tolist()
    want = ref.sample_batch(ip, ix, ew, seeds, fanouts, 0x3C6EF372)
    assert c[COUNT_STATUS(2)] == 0 and c[COUNT_INPUT(2)] == want["input_nodes"].size
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"])
    for i, (gl, wl) in enumerate(zip(got["layers"], want["layers"])):
        assert (c[COUNT_EDGES(i)], gl["num_src"], gl["num_dst"]) == (wl["row"].size, wl["num_src"], wl["num_dst"]), i
        for name in ("row", "col", "eid"):
            np.testing.assert_array_equal(host_u32(gl[name]), wl[name], err_msg=f"{name} layer {i}")
    assert ops.device_status() == 0
