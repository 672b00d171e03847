"""Every sampler kernel at edge positions past 2^30 and 2^31.

ggms_id_t is uint32: a CSR may have up to 2^32 - 1 edges, `indices + position` passes 2^32 BYTES at position 2^30, and a
position no longer fits a signed 32-bit integer from 2^31 on.  graphgen.high_offset_csr puts a small graph there: ~3000
real nodes, a hub whose 6000-neighbour list has edge position `boundary` in its middle, and one filler node whose list
(never read; its id is in no real list and no seed) pushes the hub up.  Half of the real nodes lie entirely below the
boundary, the others entirely above.  `indices` is torch.empty(E): 4.3 GB at 2^30, 8.6 GB at 2^31.

Whatever a sampler does on that graph it must do on the SHIFTED graph too -- the same CSR with the filler at degree 0 --
which is what the C oracle and the numpy references get: COO, input nodes, permuted lists and RNG pools are compared
bit for bit.  (ggms_link_seeds hashes the edge POSITION: its reference gets the real offsets and reads `indices`
through graphgen.SparseIndices.)

What these tests see that the suite did not: with GraphView::neighbours returning indices + (position & 0x7fffffff) every
sampler test that existed before this file passed (the full-size graphs have 1.62e9 and 1.8e9 edges, below 2^31), and
here the khop0, khop3, khop_labor, random-walk, batch, prefetch and closure tests at 2^31 failed.  (khop1, khop2, the
weighted samplers and ggms_link_seeds address `indices` themselves and are not reached by that one-line change.)"""
import numpy as np
import pytest

import khop_labor_ref
import link_ref
import oracle
from graphgen import high_offset_csr, high_offset_table, prefix_sums
from test_gpu_parity import dev, host_u32, states_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BITS = [30, 31]
at = pytest.mark.parametrize("bits", BITS, ids=[f"2^{b}" for b in BITS])


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def graph_at(ops):
    """graph_at(bits) = (high_offset_csr(2^bits), its DeviceGraph): built on first use, released at module end."""
    made = {}

    def get(bits):
        if bits not in made:
            g = high_offset_csr(1 << bits, seed=bits)
            assert g.num_edge > 1 << bits and g.indices.numel() == g.num_edge
            made[bits] = (g, ops.DeviceGraph(dev(g.indptr), g.indices))
        return made[bits]
    yield get
    made.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def seeds_of(g, n, rng, distinct=False):
    """n seeds: the hub, then real nodes from both sides of the boundary alternately; never the filler.  Not distinct:
    some of them repeat (the hub too)."""
    lo, hi = rng.permutation(g.below), rng.permutation(g.above)
    s = np.empty(n, np.uint32)
    s[0::2], s[1::2] = lo[:(n + 1) // 2], hi[:n // 2]
    s[0] = g.hub
    if not distinct and n > 20:
        s[7], s[11], s[n - 1] = s[3], g.hub, s[2]
    assert g.filler not in s and (s < g.filler).any() and (s > g.hub).any()
    return s


def check_leaf(got, want, what=""):
    m = int(got[-1].item())
    assert m == want[0].size, what
    for k, w in enumerate(want):
        np.testing.assert_array_equal(host_u32(got[k], m), w, err_msg=f"{what} output {k}")


def check_states(st_gpu, st_orc):
    got = states_np(st_gpu)
    np.testing.assert_array_equal(got[:, 0], st_orc["d"])
    np.testing.assert_array_equal(got[:, 1:], st_orc["v"])


# ---- leaves ----------------------------------------------------------------------------------------------------------------
LEAVES = [("khop0", 5), ("khop0", 25), ("khop0", 4000), ("khop1", 5), ("khop1", 25), ("khop2", 5), ("khop2", 25),
          ("khop3", 5), ("khop3", 25), ("khop_labor", 5), ("khop_labor", 25)]


@at
@pytest.mark.parametrize("sampler,fanout", LEAVES, ids=[f"{s}-{f}" for s, f in LEAVES])
def test_leaf_samplers(ops, graph_at, bits, sampler, fanout):
    """khop0 (fanout 4000: the hub goes through the heavy-list path, test_samplers_on_hub_graph), khop1, khop2 (distinct
    seeds; the permuted lists are compared too), khop3, khop_labor: two calls each, the RNG pool carried over."""
    g, graph = graph_at(bits)
    ip, ix = g.indptr_shifted, g.indices_shifted.copy()
    rng = np.random.RandomState(bits * 100 + fanout)
    n = 301
    inp = seeds_of(g, n, rng, distinct=sampler == "khop2")
    nstates = {"khop3": max(64, (n + 127) // 128 * 8), "khop1": max(256, min(n * fanout, 512 * 1024)),
               "khop2": max(256, (n + 1023) // 1024 * 256)}.get(sampler)
    st_gpu = ops.random_states(nstates, 31 + bits) if nstates else None
    st_orc = oracle.random_states(nstates, 31 + bits) if nstates else None
    t_inp = dev(inp)
    try:
        for rep in range(2):
            if sampler == "khop0":
                got, want = ops.sample_khop0(graph, t_inp, fanout), oracle.sample_khop0(ip, ix, inp, fanout)
            elif sampler == "khop1":
                got, want = ops.sample_khop1(graph, t_inp, fanout, st_gpu), oracle.sample_khop1(ip, ix, inp, fanout, st_orc)
            elif sampler == "khop2":
                got, want = ops.sample_khop2(graph, t_inp, fanout, st_gpu), oracle.sample_khop2(ip, ix, inp, fanout, st_orc)
            elif sampler == "khop3":
                got, want = ops.sample_khop3(graph, t_inp, fanout, st_gpu), oracle.sample_khop3(ip, ix, inp, fanout, st_orc)
            else:
                salt = 0xC0FFEE + rep
                got = ops.sample_khop_labor(graph, t_inp, fanout, salt)
                want = khop_labor_ref.sample_layer(g.indptr, g.ix, inp, fanout, salt)[1:]
            check_leaf(got, want, f"{sampler} rep {rep}")
            if st_gpu is not None:
                check_states(st_gpu, st_orc)
        if sampler == "khop2":  # the lists as the sampler permuted them, on both sides of the filler
            np.testing.assert_array_equal(host_u32(g.indices[:g.head.size]), ix[:g.head.size])
            np.testing.assert_array_equal(host_u32(g.indices[g.tail_start:]), ix[g.head.size:])
            assert not np.array_equal(ix, g.indices_shifted)
    finally:
        if sampler == "khop2":
            g.restore()
    assert ops.device_status() == 0


@pytest.mark.parametrize("fanout", [5, 25])
def test_weighted_samplers_at_2_31(ops, graph_at, fanout):
    """weighted_khop, weighted_khop_prefix and weighted_khop_hash_dedup: the prob / alias / prefix-sum tables are
    torch.empty(E) with only the real part written (26 GB together with the indices), built here and freed here."""
    g, graph = graph_at(31)
    ip, ix = g.indptr_shifted, g.indices_shifted
    total = ip.size - 1
    rng = np.random.RandomState(fanout)
    prob = rng.random_sample(ix.size).astype(np.float32)
    alias = rng.randint(0, total - 1, ix.size).astype(np.uint32)
    alias[alias >= g.filler] += 1
    pre = prefix_sums(ip, (rng.random_sample(ix.size) + 0.01).astype(np.float32))
    t_prob, t_alias, t_pre = (high_offset_table(g, a) for a in (prob, alias, pre))
    n = 301
    inp = seeds_of(g, n, rng)
    t_inp = dev(inp)
    tasks = n * fanout
    for name, nstates in (("weighted_khop", max(256, min((min(tasks, 512 * 1024) + 255) // 256 * 256, tasks))),
                          ("weighted_khop_prefix", max(256, min(tasks, 512 * 1024))),
                          ("weighted_khop_hash_dedup", max(256, (n + 1023) // 1024 * 256))):
        st_gpu, st_orc = ops.random_states(nstates, 4242), oracle.random_states(nstates, 4242)
        for rep in range(2):
            if name == "weighted_khop":
                got = ops.sample_weighted_khop(graph, t_prob, t_alias, t_inp, fanout, st_gpu)
                want = oracle.sample_weighted_khop(ip, ix, prob, alias, inp, fanout, st_orc)
            elif name == "weighted_khop_prefix":
                got = ops.sample_weighted_khop_prefix(graph, t_pre, t_inp, fanout, st_gpu)
                want = oracle.sample_weighted_khop_prefix(ip, ix, pre, inp, fanout, st_orc)
            else:
                got = ops.sample_weighted_khop_hash_dedup(graph, t_prob, t_alias, t_inp, fanout, st_gpu)
                want = oracle.sample_weighted_khop_hash_dedup(ip, ix, prob, alias, inp, fanout, st_orc)
            check_leaf(got, want, f"{name} rep {rep}")
            check_states(st_gpu, st_orc)
    assert ops.device_status() == 0
    del t_prob, t_alias, t_pre
    torch.cuda.empty_cache()


@at
def test_random_walk(ops, graph_at, bits):
    """PinSAGE walks (length 3, restart 0.5, 4 walks, top 5): every step reads a list on one side of the boundary or the
    other, or the hub's."""
    g, graph = graph_at(bits)
    ip, ix = g.indptr_shifted, g.indices_shifted
    n = 301
    inp = seeds_of(g, n, np.random.RandomState(bits))
    nstates = max(256, ops.lib().ggms_random_walk_num_states(n, 4))
    st_gpu, st_orc = ops.random_states(nstates, 777), oracle.random_states(nstates, 777)
    for rep in range(2):
        got = ops.sample_random_walk(graph, dev(inp), 3, 0.5, 4, 5, st_gpu)
        want = oracle.sample_random_walk(ip, ix, inp, 3, 0.5, 4, 5, st_orc)
        check_leaf(got, want, f"random walk rep {rep}")
        check_states(st_gpu, st_orc)
    assert ops.device_status() == 0


# ---- batch paths -------------------------------------------------------------------------------------------------------
def check_batch(got, want, L, what=""):
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"], err_msg=what)
    for i in range(L):
        gl, wl = got["layers"][i], want["layers"][i]
        assert (gl["num_src"], gl["num_dst"]) == (wl["num_src"], wl["num_dst"]), (what, i)
        np.testing.assert_array_equal(host_u32(gl["row"]), wl["row"], err_msg=f"{what} row {i}")
        np.testing.assert_array_equal(host_u32(gl["col"]), wl["col"], err_msg=f"{what} col {i}")


@at
@pytest.mark.parametrize("stype", ["khop3", "khop0"])
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_batch_sampler(ops, graph_at, bits, stype, direct):
    """ggms_sample_batch, fanouts [5, 10, 15], 300 seeds, both table layouts, seeds promised distinct and not: the
    oracle's batch on the shifted graph, and its RNG pool."""
    g, graph = graph_at(bits)
    ip, ix = g.indptr_shifted, g.indices_shifted
    fanouts = [5, 10, 15]
    code, ocode = (ops.KHOP3, oracle.KHOP3) if stype == "khop3" else (ops.KHOP0, oracle.KHOP0)
    bs = ops.BatchSampler(graph, fanouts, 300, sample_type=code, seed=77, direct_table=direct)
    orc_states = oracle.random_states(bs.states.shape[0], 77) if bs.states is not None else None
    rng = np.random.RandomState(bits + 5)
    for distinct in (True, False):
        seeds = seeds_of(g, 300, rng, distinct=distinct)
        bs.sample(dev(seeds), distinct=distinct)
        got = bs.result()
        want = oracle.do_sample(ocode, ip, ix, seeds, fanouts, orc_states)
        check_batch(got, want, 3, f"{stype} distinct={distinct}")
        assert g.hub in want["input_nodes"] and g.filler not in want["input_nodes"]
        if orc_states is not None:
            check_states(bs.states, orc_states)
    assert ops.device_status() == 0


@at
def test_prefetch_batch_sampler(ops, graph_at, bits):
    """ggms_sample_batch_prefetch (the expansion walk of edge_tiles.h reads the hub's whole list across the boundary):
    the replay test_gpu_arch4.py holds its leaf test to, on the same batch.  The host-side sizing helper gets the
    shifted offsets: the filler's degree is no list anybody expands."""
    from test_gpu_arch4 import prefetch_replay
    g, graph = graph_at(bits)
    ip, ix = g.indptr_shifted, g.indices_shifted
    fanouts = [5, 10, 15]
    bs = ops.PrefetchBatchSampler(graph, ip, fanouts, 300, sample_type=ops.KHOP0, seed=9)
    rng = np.random.RandomState(bits + 5)
    for distinct in (True, False):
        seeds = seeds_of(g, 300, rng, distinct=distinct)
        bs.sample(dev(seeds), distinct=distinct)
        got = bs.result()
        want = prefetch_replay(oracle.do_sample(oracle.KHOP0, ip, ix, seeds, fanouts, None), ip, ix)
        assert got["expansion_edges"] == want["expansion_edges"] >= 6000
        check_batch(got, want, 3, f"prefetch distinct={distinct}")
    assert ops.device_status() == 0


# ---- closure and link seeds --------------------------------------------------------------------------------------------
@at
def test_khop_closure(ops, graph_at, bits):
    """ggms_khop_closure, 2 hops from seeds on both sides and the hub: test_gpu_presample_static.py's BFS on the shifted
    graph, level by level."""
    from test_gpu_presample_static import _closure_levels, bfs_levels
    g, graph = graph_at(bits)
    ip, ix = g.indptr_shifted, g.indices_shifted
    visit = torch.zeros(ip.size - 1, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(bits)
    for stamp, n in enumerate((5, 64, 301), start=1):
        seeds = seeds_of(g, n, rng)
        got = _closure_levels(ops, graph, seeds, 2, visit, stamp)
        want = bfs_levels(ip, ix, seeds, 2)
        for h in range(3):
            np.testing.assert_array_equal(got[h], want[h], err_msg=f"hop {h}, {n} seeds")
        assert g.filler not in np.concatenate(want)
    ops.check_device_status("khop_closure")


@at
@pytest.mark.parametrize("mode", [link_ref.UNIFORM, link_ref.EXCLUDE], ids=["uniform", "exclude"])
@pytest.mark.parametrize("K", [5, 64])
def test_link_seeds(ops, graph_at, bits, K, mode):
    """ggms_link_seeds binary-searches indptr for the edge's source and reads indices[e]: edge ids just below and above
    the boundary, the hub's first, middle and last edge, the first and last real edge, the last edge below the filler
    and the first above it, repeated ids, random ids on both sides, and one id >= E."""
    g, graph = graph_at(bits)
    ip = g.indptr
    E, b, h0, h1 = g.num_edge, g.boundary, int(ip[g.hub]), int(ip[g.hub + 1])
    rng = np.random.RandomState(bits + K)
    eids = [b - 1, b, b + 1, b - 2, h0, (h0 + h1) // 2, h1 - 1, h1, 0, E - 1, g.head.size - 1, g.tail_start, b, b, 0, E + 5]
    eids += rng.randint(0, g.head.size, 40).tolist() + rng.randint(g.tail_start, E, 80).tolist()
    eids = np.array(eids, np.uint32)[rng.permutation(len(eids))]
    assert eids.size % 64 and (eids >= b).sum() > 30 and (eids < g.head.size).sum() > 30
    salt = 0xA5000000 + 131 * K + bits
    out, forced = ops.link_seeds(graph, dev(eids), K, mode, salt)
    want, want_forced = link_ref.link_seeds(ip, g.ix, eids, K, mode, salt)
    got = host_u32(out)
    for a, w, name in zip(link_ref.split(got, K), link_ref.split(want, K), ("src", "dst", "neg")):
        np.testing.assert_array_equal(a, w, err_msg=name)
    assert int(forced.item()) == want_forced and (mode == link_ref.UNIFORM or want_forced > 0)
    bad = np.flatnonzero(eids >= E)
    assert bad.size == 1 and (link_ref.split(got, K)[0][bad] == link_ref.EMPTY).all()
    assert ops.device_status() == 0
