"""ppr_topk on the GPU against its numpy statement (tests/ppr_ref.py), bit for bit: src, dst, the scores, the count and
the stats.  One graph of small components -- a path and a symmetric ring (score ties, broken by node id), a star of 70
leaves (at C = 64 its hub truncates in round 1, a leaf in round 2), a dangling node behind an edge, an isolated node,
a list with parallel edges and a self-loop -- and a power-law graph of 3000 nodes (truncation in later rounds at
C = 64, rounds that count their new keys first and fit, a full map at the largest C)."""
import numpy as np
import pytest

import ppr_ref as ref
from graphgen import powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATH, RING, HUB, LEAF, TO_DANGLING, ISOLATED, MULTI, RANDOM = 0, 9, 21, 22, 92, 94, 95, 98


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def zoo():
    lists = [[j for j in (i - 1, i + 1) if 0 <= j < 9] for i in range(9)]                 # path 0 .. 8
    lists += [[RING + (i - 1) % 12, RING + (i + 1) % 12] for i in range(12)]              # ring 9 .. 20
    lists += [list(range(LEAF, LEAF + 70))] + [[HUB]] * 70                                # star: hub 21, leaves 22 .. 91
    lists += [[TO_DANGLING + 1, TO_DANGLING], []]                                         # 92 -> {93 (dangling), 92}
    lists += [[]]                                                                         # 94: isolated
    lists += [[MULTI + 1, MULTI + 1, MULTI, MULTI + 2], [MULTI], [MULTI, MULTI + 1]]      # 95 .. 97
    rip, rix = powerlaw_csr(3000, mean_deg=8, seed=5)
    ip = np.concatenate([np.cumsum([0] + [len(l) for l in lists]), len(sum(lists, [])) + rip[1:].astype(np.int64)])
    return ip.astype(np.uint32), np.concatenate([np.array(sum(lists, []), np.uint32), rix + np.uint32(RANDOM)])


@pytest.fixture(scope="module")
def graph(ops):
    ip, ix = zoo()
    g = ops.DeviceGraph(dev(ip), dev(ix))
    yield ip, ix, g
    g.detach_heads()


SPECIAL = [PATH, PATH + 4, RING, RING + 5, HUB, LEAF, TO_DANGLING, TO_DANGLING + 1, ISOLATED, MULTI, ref.EMPTY, RING, HUB,
           RANDOM + 7]


def random_seeds(n):
    return (RANDOM + np.random.RandomState(n).randint(0, 3000, n)).tolist()


def check(ops, graph, inp, alpha, eps, C, rounds, K):
    ip, ix, g = graph
    inp = np.array(inp, np.uint32)
    src, dst, data, num, stat = ops.sample_ppr(g, dev(inp), alpha, eps, C, rounds, K)
    _, wsrc, wdst, wdata, wstat = ref.sample_layer(ip, ix, inp, alpha, eps, C, rounds, K)
    m = int(num.cpu()[0])
    assert m == wsrc.size
    for got, want in ((src, wsrc), (dst, wdst), (data, wdata)):
        np.testing.assert_array_equal(got.cpu().numpy()[:m].view(np.uint32), want)
    np.testing.assert_array_equal(stat.cpu().numpy().view(np.uint32).reshape(-1, 2), wstat)
    assert ops.device_status() == 0
    return wstat


#        seeds                alpha  eps        C     rounds K    grid cap
CASES = [(SPECIAL,            0.15,  1e-4,      64,   32,    4,   None),   # truncation in round 1 and 2, ties, dangling
         (SPECIAL,            0.15,  2.0 ** -20, 2048, 255,  127, None),   # largest C, K above the scored nodes
         (SPECIAL,            0.5,   1e-3,      128,  1,     1,   None),   # one round, K = 1
         ([],                 0.15,  1e-4,      1024, 32,    10,  None),
         ([RANDOM + 10],      0.95,  1e-4,      1024, 32,    10,  1),
         (random_seeds(65),   0.05,  1e-3,      64,   32,    10,  1),      # later grid rounds; truncation in later rounds
         (random_seeds(3),    0.15,  2.0 ** -20, 2048, 12,   100, None),   # the map fills the largest C
         (random_seeds(4),    0.3,   1e-3,      256,  32,    10,  None)]   # rounds that count their new keys and fit


@pytest.mark.parametrize("case", CASES, ids=[f"n{len(c[0])}-a{c[1]}-C{c[3]}-r{c[4]}-K{c[5]}" for c in CASES])
def test_leaf_equals_the_reference(ops, graph, case):
    from xgnn_amd import lib
    inp, alpha, eps, C, rounds, K, cap = case
    if cap:
        lib().ggms_debug_set_knob(3, cap)  # GGMS_DEBUG_GRID_CAP
    try:
        stat = check(ops, graph, inp, alpha, eps, C, rounds, K)
    finally:
        lib().ggms_debug_set_knob(3, -1)
    if inp is SPECIAL and C == 64:  # the cases are what they claim to be
        assert stat[4].tolist() == [1 << 31, 0] and stat[5, 0] == (1 << 31) | 1 and stat[8].tolist() == [1, 1 << 30]
    if C == 2048 and len(inp) == 3:
        assert (stat[:, 0] >> 31).all()


def test_batch_equals_the_reference_chain(ops, graph):
    ip, ix, g = graph
    seeds = np.array(random_seeds(20) + [RING, HUB], np.uint32)
    bs = ops.PprBatchSampler(g, 2, 3, 0.15, 1e-3, 64, 32, batch_size=len(seeds))
    bs.sample(dev(seeds))
    got, want = bs.result(), ref.sample_batch(ip, ix, seeds, 2, 0.15, 1e-3, 64, 32, 3)
    np.testing.assert_array_equal(got["input_nodes"].cpu().numpy().view(np.uint32), want["input_nodes"])
    for gl, wl in zip(got["layers"], want["layers"]):
        for name in ("row", "col", "data"):
            np.testing.assert_array_equal(gl[name].cpu().numpy().view(np.uint32), wl[name], err_msg=name)
        assert (gl["num_src"], gl["num_dst"]) == (wl["num_src"], wl["num_dst"])
