"""random_walk_metapath on the GPU against its numpy statement (tests/walk_metapath_ref.py), bit for bit: src, dst, the
visit counts and the count word (a sentinel behind it).  One graph of 400 nodes and three relations: lists of degree 0,
lists without relation 0 / 1 / 2 (a walk that ends at the first, a middle and the last step), segments of one entry,
one-relation lists, a hub of 70 000 entries whose relation-1 segment is the single entry at position 66 000 (the wave's
search, boundaries past 2^16) and a hub of one relation."""
import numpy as np
import pytest

import walk_metapath_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NODES, HUB, HUB1 = 400, 398, 399
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


@pytest.fixture(scope="module")
def graph(ops):
    rng = np.random.RandomState(12)
    counts = rng.randint(0, 5, (NODES, 3))          # entries per relation
    counts[0:40:4] = 0                              # degree 0
    counts[40:70, 0], counts[70:100, 1], counts[100:130, 2] = 0, 0, 0  # a relation the list lacks
    counts[130:160] = np.minimum(counts[130:160], 1)  # segments of one entry
    counts[160:200, 1:] = 0                         # one-relation lists
    counts[HUB], counts[HUB1] = [66_000, 1, 3_999], [3_000, 0, 0]
    ip = np.zeros(NODES + 1, np.uint32)
    ip[1:] = np.cumsum(counts.sum(1))
    ix = rng.randint(0, NODES, int(ip[-1])).astype(np.uint32)
    ix[rng.random_sample(ix.size) < 0.05] = HUB     # the walks reach the hubs from elsewhere too
    ix[rng.random_sample(ix.size) < 0.03] = HUB1
    et = np.repeat(np.tile(np.arange(3, dtype=np.uint8), NODES), counts.reshape(-1))
    g = ops.DeviceGraph(dev(ip), dev(ix))
    yield ip, ix, et, g, dev(et)
    g.detach_heads()  # the handle goes back now, not when the object is collected


def seeds_of(n, rng):
    if n == 1:
        return np.array([HUB], np.uint32)
    s = rng.randint(0, NODES, n).astype(np.uint32)
    s[0], s[1], s[n // 2] = HUB, HUB1, HUB
    s[5::17] = ref.EMPTY          # entries that yield nothing
    s[n - 20:] = s[10:30]         # repeated seeds walk identically
    return s


def check(ops, graph, inp, metapath, W, T, K, p, salt):
    ip, ix, et, g, t_et = graph
    word = torch.tensor([0, SENTINEL], dtype=torch.int64, device="cuda")
    src, dst, data, _ = ops.sample_walk_metapath(g, t_et, 3, metapath, dev(inp), T, p, W, K, salt, num_out=word[:1])
    _, wsrc, wdst, wdata = ref.sample_layer(ip, ix, et, metapath, inp, T, p, W, K, salt)
    m, behind = word.cpu().tolist()
    assert (m, behind) == (wsrc.size, SENTINEL)
    for got, want in ((src, wsrc), (dst, wdst), (data, wdata)):
        np.testing.assert_array_equal(got.cpu().numpy()[:m].view(np.uint32), want)
    assert ops.device_status() == 0
    return m


#        n   metapath    W  T   K   p
CASES = [(1, [0], 1, 1, 1, 0.0), (63, [1, 2], 4, 3, 3, 0.5), (64, [2, 1, 0], 4, 3, 64, 0.0), (65, [1, 2], 1, 1, 3, 1.0),
         (257, [2, 1, 0], 4, 3, 3, 0.5), (257, [0], 4, 3, 64, 1.0), (65, [0], 4, 3, 1, 0.5), (64, [1, 2], 4, 3, 1, 0.0),
         (63, [2, 1, 0], 1, 1, 64, 0.5), (257, [1, 2], 4, 3, 64, 0.0),
         (65, [2, 1, 0], 12, 11, 3, 0.1)]  # 132 visits per seed: the top-K's spill route fed by this producer


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c).replace(" ", "") for c in CASES])
def test_leaf_equals_the_reference(ops, graph, case):
    n, metapath, W, T, K, p = case
    inp = seeds_of(n, np.random.RandomState(n + W))
    check(ops, graph, inp, metapath, W, T, K, p, 0x9E3779B9 ^ n)


def test_leaf_later_grid_rounds(ops, graph):
    """3400 seeds under a grid cap of 3 workgroups: 54 waves' worth of seeds per walk, 12 waves per round."""
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(3, 3)  # GGMS_DEBUG_GRID_CAP
    try:
        check(ops, graph, seeds_of(3400, np.random.RandomState(3)), [2, 1, 0], 4, 3, 3, 0.25, 0xABCD)
    finally:
        lib().ggms_debug_set_knob(3, -1)
