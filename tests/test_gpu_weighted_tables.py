"""GPU: the weighted / with-replacement samplers on tables built from weights, not random ones.

The other GPU tests of ggms_sample_weighted_khop, _prefix, _hash_dedup and ggms_sample_khop1 draw `prob` in [0, 1) and
`alias` from all node ids.  Such tables never reach: the termination rule of hash_dedup (a seed that has drawn 65536
candidates takes every further one; with random alias ids a list longer than `fanout` always offers `fanout` distinct
candidates), `prob == 0` and `prob == 1` slots, plateaus in the prefix sums, a sum that stops growing in f32, lists of
length 1 - 3 under the binary search, x equal to a prefix value.  Nor do they say what the draws MEAN: here the
frequencies of the GPU's own draws are held against w / sum(w) in float64.

Every test compares src, dst, the count and the whole state pool with the oracle bit for bit, checks the properties on
the GPU's own output, and ends on a clean device status word.  tests/test_weighted_meaning_host.py shows on the oracle
alone that the inputs stay inside the bounds asserted here."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import weighted_cases as wc
from graphgen import powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:  # the shared frequency graph is read-only on the host; torch wants a writable source
        a = a.copy()
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host_u32(t, n=None):
    a = t.cpu().numpy()
    if n is not None:
        a = a[:n]
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same_as_oracle(got, want, st_gpu, st_orc, what=""):
    """(src, dst, num) of a leaf call against the oracle's (src, dst), and the pools; -> the GPU's own (src, dst)."""
    src, dst, num = got
    m = int(num.item())
    assert m == want[0].size, what
    g_src, g_dst = host_u32(src, m), host_u32(dst, m)
    np.testing.assert_array_equal(g_src, want[0], err_msg=f"src {what}")
    np.testing.assert_array_equal(g_dst, want[1], err_msg=f"dst {what}")
    np.testing.assert_array_equal(st_gpu.cpu().numpy().view(np.uint32), wc.states_rows(st_orc), err_msg=f"states {what}")
    return g_src, g_dst


def same_batch_as_oracle(got, want, num_layer, what=""):
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"], err_msg=f"input nodes {what}")
    for i in range(num_layer):
        gl, wl = got["layers"][i], want["layers"][i]
        assert (gl["num_src"], gl["num_dst"]) == (wl["num_src"], wl["num_dst"]), (what, i)
        np.testing.assert_array_equal(host_u32(gl["row"]), wl["row"], err_msg=f"row layer {i} {what}")
        np.testing.assert_array_equal(host_u32(gl["col"]), wl["col"], err_msg=f"col layer {i} {what}")


# ------------------------------------------------------------------ give-up
@pytest.mark.parametrize("variant", ["base", "after", "pair"])
@pytest.mark.parametrize("fanout", wc.GIVEUP_FANOUTS)
def test_hash_dedup_give_up_leaf(ops, fanout, variant):
    """Seeds without `fanout` distinct candidates: 4096 rounds of 16 tries that accept nothing new, then the round(s)
    in which every try is taken (fanout 17: the seed completes on that round's LAST try and the generator is not
    rewound; 5 and 16: mid-round, it is; 18, 33, 49: two, three, four such rounds).  Two calls: the second starts from
    the states a give-up leaves.  `after`: streams 0 and 1 go on to two more long lists; `pair`: nodes 0 and 1 also at
    positions 16 and 17."""
    indptr, indices, prob, alias = wc.giveup_graph(fanout)
    seeds = wc.giveup_seeds(fanout, variant)
    g = ops.DeviceGraph(dev(indptr), dev(indices))
    t_prob, t_alias, t_seeds = dev(prob), dev(alias), dev(seeds)
    n = wc.stream_states(seeds.size)
    st_gpu, st_orc = ops.random_states(n, 0x1001), oracle.random_states(n, 0x1001)
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ops.sample_weighted_khop_hash_dedup(g, t_prob, t_alias, t_seeds, fanout, st_gpu)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        want = oracle.sample_weighted_khop_hash_dedup(indptr, indices, prob, alias, seeds, fanout, st_orc)
        g_src, g_dst = same_as_oracle(got, want, st_gpu, st_orc, f"call {rep}")
        wc.check_giveup_output(fanout, seeds, indptr, g_src, g_dst)
        print(f"give-up leaf, fanout {fanout}, {variant}, {seeds.size} seeds, call {rep}: {dt * 1e3:.2f} ms")
    assert ops.device_status() == 0


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("fanouts", [[5], [17, 5]])
def test_hash_dedup_give_up_batch(ops, fanouts, direct):
    """The same seeds through ggms_sample_batch: a give-up seed emits duplicate ids into the batch's dedup table
    (direct and hashed); input nodes and local ids are the oracle's.  [17, 5]: nodes 0 - 2 give up in both layers."""
    indptr, indices, prob, alias = wc.giveup_graph(fanouts[0])
    g = ops.DeviceGraph(dev(indptr), dev(indices))
    bs = ops.BatchSampler(g, fanouts, 300, sample_type=ops.WEIGHTED_KHOP_HASH_DEDUP, seed=0x1001, direct_table=direct,
                          prob_table=dev(prob), alias_table=dev(alias))
    st_orc = oracle.random_states(bs.states.shape[0], 0x1001)
    for rep, variant in enumerate(["base", "pair"]):
        seeds = wc.giveup_seeds(fanouts[0], variant)
        bs.sample(dev(seeds))
        got = bs.result()
        want = oracle.do_sample(oracle.WEIGHTED_KHOP_HASH_DEDUP, indptr, indices, seeds, fanouts, st_orc, prob=prob,
                                alias=alias)
        same_batch_as_oracle(got, want, len(fanouts), f"batch {rep}")
        np.testing.assert_array_equal(bs.states.cpu().numpy().view(np.uint32), wc.states_rows(st_orc))
        # the seeds' layer on the GPU's own output: node 0 (local id 0) has `fanout` edges, all to one node
        last = got["layers"][-1]
        row, col = host_u32(last["row"]), host_u32(last["col"])
        assert np.count_nonzero(col == 0) >= fanouts[-1] and np.unique(row[col == 0]).size == 1
    assert ops.device_status() == 0


# --------------------------- the batch path of the two samplers the other batch tests leave out
@pytest.fixture(scope="module")
def weighted_graph():
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    w = datagen.edge_weights(dict(indptr=ip, indices=ix), "default")
    prob, alias = oracle.create_alias_table(ip, ix, w)
    return ip, ix, prob, alias, oracle.create_prob_prefix_table(ip, w)


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("stype", ["prefix", "hash_dedup"])
def test_sample_batch_prefix_and_hash_dedup(ops, weighted_graph, stype, direct):
    ip, ix, prob, alias, prefix = weighted_graph
    N = ip.size - 1
    g = ops.DeviceGraph(dev(ip), dev(ix))
    fanouts = [10, 5]
    if stype == "prefix":
        bs = ops.BatchSampler(g, fanouts, 500, sample_type=ops.WEIGHTED_KHOP_PREFIX, seed=5, direct_table=direct,
                              prob_table=dev(prefix))
        code, kw = oracle.WEIGHTED_KHOP_PREFIX, dict(prob=prefix)
    else:
        bs = ops.BatchSampler(g, fanouts, 500, sample_type=ops.WEIGHTED_KHOP_HASH_DEDUP, seed=5, direct_table=direct,
                              prob_table=dev(prob), alias_table=dev(alias))
        code, kw = oracle.WEIGHTED_KHOP_HASH_DEDUP, dict(prob=prob, alias=alias)
    st_orc = oracle.random_states(bs.states.shape[0], 5)
    rng = np.random.RandomState(11)
    for rep in range(2):
        seeds = rng.permutation(N)[:500].astype(np.uint32)
        bs.sample(dev(seeds))
        same_batch_as_oracle(bs.result(), oracle.do_sample(code, ip, ix, seeds, fanouts, st_orc, **kw), 2, f"batch {rep}")
        np.testing.assert_array_equal(bs.states.cpu().numpy().view(np.uint32), wc.states_rows(st_orc))
    assert ops.device_status() == 0


# ------------------------------------------------------------------ frequencies
@pytest.fixture(scope="module")
def freq_dev(ops):
    g = wc.freq_graph()
    return SimpleNamespace(graph=ops.DeviceGraph(dev(g.indptr), dev(g.indices)), prob=dev(g.prob), alias=dev(g.alias),
                           prefix=dev(g.prefix), seeds=dev(np.arange(g.M, dtype=np.uint32)))


def _freq_gpu_call(ops, d, kind, fanout, states):
    if kind == "alias":
        return ops.sample_weighted_khop(d.graph, d.prob, d.alias, d.seeds, fanout, states)
    if kind == "prefix":
        return ops.sample_weighted_khop_prefix(d.graph, d.prefix, d.seeds, fanout, states)
    if kind == "khop1":
        return ops.sample_khop1(d.graph, d.seeds, fanout, states)
    return ops.sample_weighted_khop_hash_dedup(d.graph, d.prob, d.alias, d.seeds, fanout, states)


@pytest.mark.parametrize("kind,fanout", wc.FREQ_CONFIGS)
def test_draw_frequencies_leaf(ops, freq_dev, kind, fanout):
    """16384 seeds with one shared 24-neighbour list, warmed streams, 4 calls: bit-equal to the oracle, and the GPU's
    own counted draws within 5 binomial standard deviations of trials * w / sum(w); no zero-weight neighbour at all."""
    st_orc = wc.warmed_states(wc.freq_num_states(kind, fanout), 2024)
    st_gpu = wc.states_tensor(st_orc)
    outs = []
    for rep in range(wc.FREQ_CALLS):
        got = _freq_gpu_call(ops, freq_dev, kind, fanout, st_gpu)
        outs.append(same_as_oracle(got, wc.freq_oracle_call(kind, fanout, st_orc), st_gpu, st_orc, f"call {rep}"))
    wc.check_frequencies(kind, fanout, outs, "GPU leaf")
    assert ops.device_status() == 0


@pytest.mark.parametrize("kind,fanout", [("alias", 4), ("prefix", 4), ("khop1", 4), ("hash_dedup", 5)])
def test_draw_frequencies_batch(ops, freq_dev, kind, fanout):
    """The same through ggms_sample_batch (one layer), the batch's pool overwritten with warmed states; the global ids
    behind the GPU's local ones are counted."""
    g = wc.freq_graph()
    code = dict(alias=ops.WEIGHTED_KHOP, prefix=ops.WEIGHTED_KHOP_PREFIX, khop1=ops.KHOP1,
                hash_dedup=ops.WEIGHTED_KHOP_HASH_DEDUP)[kind]
    ocode = dict(alias=oracle.WEIGHTED_KHOP, prefix=oracle.WEIGHTED_KHOP_PREFIX, khop1=oracle.KHOP1,
                 hash_dedup=oracle.WEIGHTED_KHOP_HASH_DEDUP)[kind]
    tables = dict(alias=(freq_dev.prob, freq_dev.alias), prefix=(freq_dev.prefix, None), khop1=(None, None),
                  hash_dedup=(freq_dev.prob, freq_dev.alias))[kind]
    kw = dict(alias=dict(prob=g.prob, alias=g.alias), prefix=dict(prob=g.prefix), khop1={},
              hash_dedup=dict(prob=g.prob, alias=g.alias))[kind]
    bs = ops.BatchSampler(freq_dev.graph, [fanout], g.M, sample_type=code, seed=1, prob_table=tables[0],
                          alias_table=tables[1])
    st_orc = wc.warmed_states(bs.states.shape[0], 2024)
    bs.states.copy_(wc.states_tensor(st_orc))
    seeds = np.arange(g.M, dtype=np.uint32)
    outs = []
    for rep in range(wc.FREQ_CALLS):
        bs.sample(freq_dev.seeds)
        got = bs.result()
        same_batch_as_oracle(got, oracle.do_sample(ocode, g.indptr, g.indices, seeds, [fanout], st_orc, **kw), 1,
                             f"batch {rep}")
        np.testing.assert_array_equal(bs.states.cpu().numpy().view(np.uint32), wc.states_rows(st_orc))
        nodes = host_u32(got["input_nodes"])
        outs.append((nodes[host_u32(got["layers"][0]["col"])], nodes[host_u32(got["layers"][0]["row"])]))
    wc.check_frequencies(kind, fanout, outs, "GPU batch")
    assert ops.device_status() == 0


# ------------------------------------------------------------------ prefix-sum edges
@pytest.mark.parametrize("fanout", [1, 3])
def test_prefix_table_edges(ops, fanout):
    """Each list of weighted_cases.prefix_edge_lists owned by 512 seeds: bit-equal, and on the GPU's output no
    zero-weight position (all-zero list: position 0, the defined result of `x <= prefix[first]`), only position 0 where
    the f32 sums stop at 2^24, only the two ends of [3, 0, 0, 0, 0, 0, 0, 2]."""
    for w in wc.prefix_edge_lists():
        g = wc.shared_list_graph(wc.PREFIX_M, w)
        dg = ops.DeviceGraph(dev(g.indptr), dev(g.indices))
        t_pre, t_inp = dev(g.prefix), dev(np.arange(g.M, dtype=np.uint32))
        n = wc.task_states(g.M * fanout)
        st_gpu, st_orc = ops.random_states(n, 31), oracle.random_states(n, 31)
        for rep in range(2):
            got = ops.sample_weighted_khop_prefix(dg, t_pre, t_inp, fanout, st_gpu)
            want = oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, np.arange(g.M, dtype=np.uint32),
                                                      fanout, st_orc)
            g_src, g_dst = same_as_oracle(got, want, st_gpu, st_orc, f"weights {w[:10]} call {rep}")
            wc.check_prefix_output(w, g_dst, g.M)
    assert ops.device_status() == 0


def test_prefix_tie_goes_to_the_position_that_ends_there(ops):
    """u * total == prefix[j] exactly (hand-made states uploaded as the pool): position j, on the GPU's own output."""
    g = wc.shared_list_graph(wc.PREFIX_M, wc.TIE_W)
    dg = ops.DeviceGraph(dev(g.indptr), dev(g.indices))
    inp = np.arange(g.M, dtype=np.uint32)
    st_orc = wc.tie_states(wc.task_states(g.M))
    st_gpu = wc.states_tensor(st_orc)
    got = ops.sample_weighted_khop_prefix(dg, dev(g.prefix), dev(inp), 1, st_gpu)
    want = oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, inp, 1, st_orc)
    g_src, g_dst = same_as_oracle(got, want, st_gpu, st_orc)
    assert np.array_equal(g_src, inp)
    assert np.array_equal(g_dst.astype(np.int64) - g.M, np.arange(g.M) % 8)
    assert ops.device_status() == 0
