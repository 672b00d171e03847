"""The pair ids of a link-prediction batch: an endpoint list with heavy duplication goes through ggms_sample_batch
with seeds_distinct = 0, and BatchSampler.seed_ids() (ggms_sample_batch_seed_ids) hands back the local id of every
entry -- first-occurrence ranks, rows of the batch's input nodes, the ids the first sampled layer's col is made of."""
import numpy as np
import pytest

import link_ref as ref
from xgnn_amd._lib import COUNT_STATUS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FANOUTS = [3, 2]
K = 3


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


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def graph(ops):
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(2000, mean_deg=12, seed=9)
    return ip, ix, ops.DeviceGraph(dev(ip), dev(ix))


def endpoints_of(ops, ip, ix, g, rep):
    """100 positives drawn from 30 edges of 6 sources (sources, destinations and negatives repeat), K negatives each:
    the list ggms_link_seeds writes, checked against the reference on the way."""
    rng = np.random.RandomState(100 + rep)
    rows = rng.permutation(np.flatnonzero(np.diff(ip.astype(np.int64)) >= 5))[:6]
    pool = np.concatenate([np.arange(ip[v], ip[v] + 5) for v in rows])
    eids = pool[rng.randint(0, pool.size, 100)].astype(np.uint32)
    out, _ = ops.link_seeds(g, dev(eids), K, ref.EXCLUDE, 40 + rep)
    want, _ = ref.link_seeds(ip, ix, eids, K, ref.EXCLUDE, 40 + rep)
    np.testing.assert_array_equal(host_u32(out), want)
    return out, want


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("name", ["khop3", "khop0", "khop_labor"])
def test_seed_ids_are_the_first_occurrence_ranks(ops, graph, name, direct):
    ip, ix, g = graph
    code = {"khop3": ops.KHOP3, "khop0": ops.KHOP0, "khop_labor": ops.KHOP_LABOR}[name]
    n = 100 * (2 + K)
    bs = ops.BatchSampler(g, FANOUTS, n, sample_type=code, seed=5, direct_table=direct)
    L = len(FANOUTS)
    kept = []
    for rep in range(2):  # the second batch runs on the same table and workspace: its ids are its own
        seeds_dev, seeds = endpoints_of(ops, ip, ix, g, rep)
        assert np.unique(seeds).size < seeds.size // 2  # heavy duplication
        bs.sample(seeds_dev, distinct=False, labor_salt=rep)
        ids = host_u32(bs.seed_ids().clone())
        got = bs.result()
        assert bs.counts.cpu().tolist()[COUNT_STATUS(L)] == 0
        want_ids, uniq = ref.first_occurrence_ranks(seeds)
        np.testing.assert_array_equal(ids, want_ids)
        nodes = host_u32(got["input_nodes"])
        np.testing.assert_array_equal(nodes[:uniq.size], uniq)  # the distinct seeds head the batch's node list
        np.testing.assert_array_equal(nodes[ids], seeds)
        # the first sampled layer (layer L - 1) samples from the raw seeds: its col is made of the same ids, one run of
        # at most fanout edges per seed position with neighbours, in seed order
        first = got["layers"][L - 1]
        col = host_u32(first["col"])
        assert first["num_dst"] == seeds.size and col.size > 0
        deg = (ip[seeds.astype(np.int64) + 1] - ip[seeds.astype(np.int64)]).astype(np.int64)
        want_col = np.repeat(want_ids, np.minimum(deg, FANOUTS[L - 1]))
        np.testing.assert_array_equal(col, want_col)
        # and every edge's row is a neighbour of its col's node
        row = nodes[host_u32(first["row"])]
        for r, c in zip(row[:200].tolist(), nodes[col[:200]].tolist()):
            assert r in ix[ip[c]:ip[c + 1]]
        kept.append(ids)
    assert not np.array_equal(kept[0], kept[1])


def test_seed_ids_need_a_non_distinct_batch(ops, graph):
    from xgnn_amd._lib import GgmsError
    ip, ix, g = graph
    bs = ops.BatchSampler(g, FANOUTS, 64, sample_type=ops.KHOP0)
    with pytest.raises(GgmsError):
        bs.seed_ids()
    bs.sample(dev(np.arange(64, dtype=np.uint32)), distinct=True)
    with pytest.raises(GgmsError):
        bs.seed_ids()
    bs.sample(dev(np.arange(64, dtype=np.uint32)), distinct=False)
    np.testing.assert_array_equal(host_u32(bs.seed_ids()), np.arange(64))
