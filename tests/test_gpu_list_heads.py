"""Inline list heads on the GPU (include/ggms.h, "Inline list heads"; list_heads.hip, k_khop3_fused<.., HEADS>).

  table    ggms_list_heads_build against a numpy-built table, byte for byte, on a hand-made CSR whose degrees sit on both
           sides of every rule: 0, 1, 14, 15 (inline), 16, 17, 64, 300 (degree + offset) -- and a node count that is no
           multiple of 128 (a khop3 tile) nor of 64; and on a graph of ONE node.
  khop3    the leaf call and ggms_sample_batch with heads attached and without: edges, order, counts and the RNG state
           pool are the same bytes, and they are the oracle's.  Fanouts 1, 5 (< 15: the inline words have LDS of their
           own, and a seed of degree 14 or 15 both draws and reads them), 15 (the boundary: the words share the positions'
           LDS), 16, 20; seed counts 1, 127, 129, 300 (one lane, a tile less one, a tile plus one, three tiles with a
           partial last one); random seeds with repeats and distinct ones (the batch's fused first layer).
  rounds   once under the grid cap (one workgroup for three tiles and more): the ticket path, LDS reused by the next tile;
           the build kernel's later rounds under caps 1 and 3.
  khop0    a sampler that does not look at the heads gives the same output with them attached."""
import ctypes as C

import numpy as np
import pytest

import oracle
import test_gpu_parity as P
import test_gpu_variants as V
from xgnn_amd._lib import COUNTS_SAMPLE_WORDS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = 601
DEGREES = (0, 1, 14, 15, 16, 17, 64, 300)
FANOUTS = (1, 5, 15, 16, 20)
SEED_COUNTS = (1, 127, 129, 300)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as o
    return o


def handmade_csr():
    """601 nodes; node v has degree DEGREES[v % 8], except that every 37th node takes a random degree in 2 .. 13."""
    rng = np.random.RandomState(601)
    deg = np.array([DEGREES[v % len(DEGREES)] for v in range(N)], dtype=np.int64)
    odd = np.arange(5, N, 37)
    deg[odd] = rng.randint(2, 14, odd.size)
    ip = np.zeros(N + 1, dtype=np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, N, int(ip[-1])).astype(np.uint32)
    return ip, ix


def numpy_heads(ip, ix):
    n = ip.size - 1
    t = np.zeros((n, 16), dtype=np.uint32)
    for v in range(n):
        b, e = int(ip[v]), int(ip[v + 1])
        t[v, 0] = e - b
        if e - b <= 15:
            t[v, 1:1 + e - b] = ix[b:e]
        else:
            t[v, 1] = b
    return t


@pytest.fixture(scope="module")
def csr(ops):
    """(indptr, indices, graph with heads, graph without) -- the two graphs share their device arrays."""
    ip, ix = handmade_csr()
    t_ip, t_ix = P.dev(ip), P.dev(ix)
    with_heads = ops.DeviceGraph(t_ip, t_ix, inline_heads=True)
    without = ops.DeviceGraph(t_ip, t_ix, inline_heads=False)
    assert with_heads.heads is not None and with_heads.c.heads_id != 0
    assert without.heads is None and without.c.heads_id == 0
    return ip, ix, with_heads, without


def seeds_of(n, distinct, salt):
    rng = np.random.RandomState(1000 * salt + n)
    if distinct:
        return rng.permutation(N)[:n].astype(np.uint32)
    s = rng.randint(0, N, n).astype(np.uint32)
    if n > 2:
        s[n // 2] = s[0]  # at least one repeat
    return s


def test_built_table_equals_numpy(ops, csr):
    ip, ix, g, _ = csr
    assert sorted(set(np.diff(ip.astype(np.int64)).tolist()) & set(DEGREES)) == sorted(DEGREES)
    assert g.heads.numel() * 4 == 64 * N and g.heads.data_ptr() % 64 == 0
    got = g.heads.cpu().numpy().view(np.uint32).reshape(N, 16)
    assert got.tobytes() == numpy_heads(ip, ix).tobytes()
    from xgnn_amd import lib
    assert lib().ggms_list_heads_of(C.byref(g.c)) == g.heads.data_ptr()


def test_built_table_of_one_node(ops):
    for deg in (0, 3, 15, 16):
        ip = np.array([0, deg], dtype=np.uint32)
        ix = np.arange(7, 7 + max(deg, 1), dtype=np.uint32)
        g = ops.DeviceGraph(P.dev(ip), P.dev(ix), inline_heads=True)
        got = g.heads.cpu().numpy().view(np.uint32).reshape(1, 16)
        assert got.tobytes() == numpy_heads(ip, ix[:deg]).tobytes(), deg


def test_default_builds_heads_and_detach_releases_them(ops):
    ip, ix = handmade_csr()
    g = ops.DeviceGraph(P.dev(ip), P.dev(ix))  # 38 KB: far below a quarter of free memory
    assert g.heads is not None and g.c.heads_id != 0
    g.detach_heads()
    assert g.heads is None and g.c.heads_id == 0
    with pytest.raises(Exception):
        ops.DeviceGraph(None, None, part_indptr=[P.dev(ip), P.dev(ip)], part_indices=[P.dev(ix), P.dev(ix)],
                        num_cache_node=0, inline_heads=True)


def leaf_case(ops, csr, n, fanout, distinct):
    ip, ix, g_heads, g_plain = csr
    seeds = seeds_of(n, distinct, fanout)
    nstates = max(64, (n + 127) // 128 * 8)
    st = [ops.random_states(nstates, 0x5EED + fanout) for _ in range(2)]
    st_orc = oracle.random_states(nstates, 0x5EED + fanout)
    t_seeds = P.dev(seeds)
    for rep in range(2):  # the pool persists across calls
        wsrc, wdst = oracle.sample_khop3(ip, ix, seeds, fanout, st_orc)
        outs = []
        for g, s in ((g_heads, st[0]), (g_plain, st[1])):
            src, dst, num = ops.sample_khop3(g, t_seeds, fanout, s)
            m = int(num.item())
            outs.append((m, P.host_u32(src, m).tobytes(), P.host_u32(dst, m).tobytes(), P.states_np(s).tobytes()))
        what = f"n {n} fanout {fanout} distinct {distinct} rep {rep}"
        assert outs[0] == outs[1], what
        m, src, dst, pool = outs[0]
        assert m == wsrc.size and src == wsrc.tobytes() and dst == wdst.tobytes(), what
        assert pool == np.concatenate([st_orc["d"][:, None], st_orc["v"]], axis=1).astype(np.uint32).tobytes(), what


@pytest.mark.parametrize("fanout", FANOUTS)
def test_khop3_leaf_with_and_without_heads(ops, csr, fanout):
    for n in SEED_COUNTS:
        for distinct in (False, True):
            leaf_case(ops, csr, n, fanout, distinct)
    assert ops.device_status() == 0


def batch_case(ops, csr, n, fanouts, distinct):
    ip, ix, g_heads, g_plain = csr
    L = len(fanouts)
    bss = [ops.BatchSampler(g, fanouts, n, sample_type=ops.KHOP3, seed=31) for g in (g_heads, g_plain)]
    st_orc = oracle.random_states(bss[0].states.shape[0], 31)
    for rep in range(2):
        seeds = seeds_of(n, distinct, 7 * fanouts[0] + rep)
        want = oracle.do_sample(oracle.KHOP3, ip, ix, seeds, fanouts, st_orc)
        outs = []
        for bs in bss:
            bs.sample(P.dev(seeds), distinct=distinct)
            r = bs.result()
            counts = bs.counts.cpu().numpy()[:COUNTS_SAMPLE_WORDS(L)]
            outs.append(dict(input_nodes=P.host_u32(r["input_nodes"]).tobytes(), counts=counts.tobytes(),
                             pool=P.states_np(bs.states).tobytes(),
                             row=[P.host_u32(l["row"]).tobytes() for l in r["layers"]],
                             col=[P.host_u32(l["col"]).tobytes() for l in r["layers"]],
                             sizes=[(l["num_src"], l["num_dst"]) for l in r["layers"]]))
        what = f"n {n} fanouts {fanouts} distinct {distinct} rep {rep}"
        assert outs[0] == outs[1], what
        o = outs[0]
        assert o["input_nodes"] == want["input_nodes"].tobytes(), what
        for i in range(L):
            wl = want["layers"][i]
            assert o["sizes"][i] == (wl["num_src"], wl["num_dst"]), (what, i)
            assert o["row"][i] == wl["row"].tobytes() and o["col"][i] == wl["col"].tobytes(), (what, i)
        assert o["pool"] == np.concatenate([st_orc["d"][:, None], st_orc["v"]], axis=1).astype(np.uint32).tobytes(), what


@pytest.mark.parametrize("fanout", FANOUTS)
def test_khop3_batch_with_and_without_heads(ops, csr, fanout):
    # the second entry is the FIRST layer processed (the seeds' layer): every fanout takes both places across the cases
    other = FANOUTS[(FANOUTS.index(fanout) + 2) % len(FANOUTS)]
    for n in SEED_COUNTS:
        batch_case(ops, csr, n, [other, fanout], distinct=False)
        batch_case(ops, csr, n, [other, fanout], distinct=True)
    assert ops.device_status() == 0


def test_khop3_later_rounds_under_the_grid_cap(ops, csr):
    """One workgroup takes every tile from the ticket: phase 1's LDS words (inline lists included) are rewritten tile
    after tile.  300 seeds are three tiles; the batch's second layer has more."""
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(V.GRID_CAP, 1)
    try:
        for fanout in (5, 16):
            leaf_case(ops, csr, 300, fanout, distinct=False)
        batch_case(ops, csr, 300, [15, 5], distinct=False)
        batch_case(ops, csr, 300, [5, 20], distinct=False)
    finally:
        lib().ggms_debug_set_knob(V.GRID_CAP, -1)
    assert ops.device_status() == 0


@pytest.mark.parametrize("cap", [1, 3])
def test_build_later_rounds_under_the_grid_cap(ops, cap):
    """k_list_heads_build takes 256 quarter records (64 nodes) per workgroup round: 601 nodes are 10 rounds for one
    workgroup, 4 for three with a partial last one."""
    from xgnn_amd import lib
    ip, ix = handmade_csr()
    lib().ggms_debug_set_knob(V.GRID_CAP, cap)
    try:
        g = ops.DeviceGraph(P.dev(ip), P.dev(ix), inline_heads=True)
        got = g.heads.cpu().numpy().view(np.uint32).reshape(N, 16)
    finally:
        lib().ggms_debug_set_knob(V.GRID_CAP, -1)
    assert got.tobytes() == numpy_heads(ip, ix).tobytes()


def test_khop0_ignores_the_heads(ops, csr):
    ip, ix, g_heads, g_plain = csr
    for n, fanout in ((129, 5), (300, 16)):
        seeds = seeds_of(n, False, fanout)
        wsrc, wdst = oracle.sample_khop0(ip, ix, seeds, fanout)
        outs = []
        for g in (g_heads, g_plain):
            src, dst, num = ops.sample_khop0(g, P.dev(seeds), fanout)
            m = int(num.item())
            outs.append((m, P.host_u32(src, m).tobytes(), P.host_u32(dst, m).tobytes()))
        assert outs[0] == outs[1] == (wsrc.size, wsrc.tobytes(), wdst.tobytes()), (n, fanout)
