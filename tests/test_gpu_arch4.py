"""arch4 on the GPU: the prefetching batch sampler (ggms_sample_batch_prefetch), the dynamic_cache gather and publish,
and the engine end to end, each against a numpy replay built on the oracle's plain batch with the same RNG pool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from test_engine import make_dataset
from xgnn_amd._lib import COUNT_EXPANSION

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER4 = os.path.join(ROOT, "tests", "arch4_driver.py")
FORCED = dict(os.environ, SAMGRAPH_FORCE_DEVICE="0")
UNFORCED = {k: v for k, v in os.environ.items() if k != "SAMGRAPH_FORCE_DEVICE"}
CODE = {"khop0": oracle.KHOP0, "khop1": oracle.KHOP1, "weighted_khop": oracle.WEIGHTED_KHOP}


def prefetch_replay(res, ip, ix):
    """arch4's batch from the plain batch `res` (oracle.do_sample, same seeds and RNG pool): the input-node prefix after
    the second-to-last layer, then every neighbour of it in first-occurrence order; the last layer's row ids remapped
    into that list, every other array unchanged."""
    ip, ix = ip.astype(np.int64), ix.astype(np.uint32)
    N = ip.size - 1
    k = int(res["layers"][1]["num_src"])
    inp = res["input_nodes"].astype(np.uint32)
    base = inp[:k]
    lists = np.concatenate([ix[ip[v]:ip[v + 1]] for v in base] + [np.zeros(0, np.uint32)])
    _, first = np.unique(lists, return_index=True)
    new = lists[np.sort(first)]
    seen = np.zeros(N, bool)
    seen[base] = True
    sup = np.concatenate([base, new[~seen[new]]]).astype(np.uint32)
    pos = np.full(N, -1, np.int64)
    pos[sup] = np.arange(sup.size)
    layers = [dict(l) for l in res["layers"]]
    layers[0]["row"] = pos[inp[res["layers"][0]["row"].astype(np.int64)]].astype(np.uint32)
    layers[0]["num_src"] = sup.size
    return dict(layers=layers, input_nodes=sup, expansion_edges=lists.size, k=k)


def _csr(N, rs, mean_deg=6, hub=None, hub_deg=0, isolated=0, dup=False):
    deg = rs.poisson(mean_deg, N)
    if isolated:
        deg[rs.choice(N, isolated, replace=False)] = 0
    if hub is not None:
        deg[hub] = hub_deg
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = rs.randint(0, N, ip[-1]).astype(np.uint32)
    if dup:  # every list repeats its first neighbour
        for v in range(N):
            if deg[v] > 1:
                ix[ip[v] + 1] = ix[ip[v]]
    return ip, ix


def _device_graph(ip, ix, dev):
    from xgnn_amd import ops
    t = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)  # noqa: E731
    return ops.DeviceGraph(t(ip), t(ix))


def _tables(ip, ix):
    from xgnn_amd import datagen
    g = dict(indptr=ip, indices=ix, train_set=np.zeros(1, np.uint32), meta=dict(feat_dim=1, num_class=1))
    return datagen.build_alias_tables(ip, ix, datagen.edge_weights(g, "default", seed=4))


LEAF = [  # (name, sample type, N, graph kwargs, fanouts, seeds)
    ("random-khop0", "khop0", 5000, dict(), [5, 4], 300),
    ("random-khop1", "khop1", 5000, dict(), [5, 4, 3], 100),
    ("random-weighted", "weighted_khop", 4000, dict(), [4, 3], 200),
    ("hub-khop0", "khop0", 3000, dict(hub=7, hub_deg=300_000), [5, 4], 200),
    ("hub-khop1", "khop1", 3000, dict(hub=11, hub_deg=100_000), [3, 3, 2], 50),
    ("isolated-dup-khop0", "khop0", 4000, dict(isolated=1500, dup=True), [5, 4], 400),
    ("isolated-dup-weighted", "weighted_khop", 3000, dict(isolated=800, dup=True), [6, 3], 150),
]


def _batch_equals_the_replay(bs, code, ip, ix, seeds, fan, states, kw, distinct, trial):
    """One batch of `bs` against prefetch_replay of the oracle's plain batch (which advances `states`); returns the
    replay."""
    bs.sample(torch.from_numpy(seeds.view(np.int32)).to(bs.counts.device), distinct=distinct)
    got = bs.result()
    want = prefetch_replay(oracle.do_sample(code, ip, ix, seeds, fan, states, **kw), ip, ix)
    assert got["expansion_edges"] == want["expansion_edges"]
    np.testing.assert_array_equal(got["input_nodes"].cpu().numpy().view(np.uint32), want["input_nodes"])
    for i, w in enumerate(want["layers"]):
        g = got["layers"][i]
        np.testing.assert_array_equal(g["row"].cpu().numpy().view(np.uint32), w["row"], err_msg=f"row{i} {trial}")
        np.testing.assert_array_equal(g["col"].cpu().numpy().view(np.uint32), w["col"], err_msg=f"col{i} {trial}")
        assert (g["num_src"], g["num_dst"]) == (w["num_src"], w["num_dst"]), (i, trial)
    if states is not None:
        assert bs.states.cpu().numpy().tobytes() == states.tobytes(), trial
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAF, ids=[c[0] for c in LEAF])
def test_prefetch_sampler_equals_the_replay(case):
    """COO of every layer, num_src / num_dst, the input nodes (superset) and the RNG pool after the batch, for distinct
    and for non-distinct seeds."""
    from xgnn_amd import ops
    name, st, N, gk, fan, ns = case
    rs = np.random.RandomState(len(name))
    dev = torch.device("cuda", 0)
    hub = gk.get("hub")
    ip, ix = _csr(N, rs, **gk)
    graph = _device_graph(ip, ix, dev)
    kw, tabs = {}, {}
    if st == "weighted_khop":
        prob, alias = _tables(ip, ix)
        kw = dict(prob=prob, alias=alias)
        tabs = dict(prob_table=torch.from_numpy(prob).to(dev), alias_table=torch.from_numpy(alias.view(np.int32)).to(dev))
    bs = ops.PrefetchBatchSampler(graph, ip, fan, ns, sample_type=CODE[st], seed=9, device=dev, **tabs)
    states = oracle.random_states(bs.states.shape[0], 9) if bs.states is not None else None
    for trial, distinct in enumerate([True, False, True]):
        seeds = rs.permutation(N)[:ns].astype(np.uint32) if distinct else rs.randint(0, N, ns).astype(np.uint32)
        if hub is not None and hub not in seeds:  # (a distinct list must not get it twice)
            seeds[0] = hub
        _batch_equals_the_replay(bs, CODE[st], ip, ix, seeds, fan, states, kw, distinct, trial)


def _csr_of(N, lists):
    """CSR of N nodes from {node: neighbours}; every other node has no list."""
    deg = np.zeros(N, np.int64)
    for v, nb in lists.items():
        deg[v] = len(nb)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    ix = np.concatenate([np.asarray(lists[v], np.uint32) for v in sorted(lists)] + [np.zeros(0, np.uint32)])
    return ip, ix


def _empty_run():
    """Seeds in order: a node of degree 1, 3000 nodes without a list, a node of degree 3.  With distinct seeds the
    unique list starts in seed order, so the expansion's first (and only) edge tile meets a run of empty lists longer
    than the walk stages at once: the tile takes a second round."""
    rs = np.random.RandomState(21)
    lists = {0: [3500], 3001: [3600, 3601, 3602]}
    lists.update({v: rs.randint(3002, 4000, 4) for v in range(3002, 4000)})
    ip, ix = _csr_of(4000, lists)
    return ip, ix, np.arange(3002, dtype=np.uint32)


def _no_edges():
    """Every seed without a list: the expansion has no edge at all."""
    rs = np.random.RandomState(22)
    ip, ix = _csr_of(300, {v: rs.randint(0, 300, 3) for v in range(100, 300)})
    return ip, ix, np.arange(100, dtype=np.uint32)


def _full_tiles():
    """512 seeds of degree 8 whose neighbours are seeds: the expansion is exactly two full edge tiles."""
    rs = np.random.RandomState(23)
    ip, ix = _csr_of(600, {v: rs.randint(0, 512, 8) for v in range(512)})
    return ip, ix, np.arange(512, dtype=np.uint32)


WALK = [("empty-run", _empty_run, None), ("no-edges", _no_edges, 0), ("full-tiles", _full_tiles, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WALK, ids=[c[0] for c in WALK])
def test_prefetch_expansion_walk_edge_cases(case):
    """khop0, two layers, seeds in a fixed order: a second round inside an edge tile, an expansion without edges, and
    one that ends exactly on a tile boundary -- each equal to the replay, with and without the distinct-seed promise."""
    from xgnn_amd import ops
    _, make, edges = case
    ip, ix, seeds = make()
    dev = torch.device("cuda", 0)
    bs = ops.PrefetchBatchSampler(_device_graph(ip, ix, dev), ip, [5, 4], seeds.size, sample_type=ops.KHOP0, seed=9,
                                  device=dev)
    for trial, distinct in enumerate([True, False]):
        want = _batch_equals_the_replay(bs, oracle.KHOP0, ip, ix, seeds, [5, 4], None, {}, distinct, trial)
        if edges is not None:
            assert want["expansion_edges"] == edges
        else:  # the run of empty lists sits inside the list that is expanded, before its last edges
            assert want["k"] > 3002 and 4 < want["expansion_edges"] < 2048


@pytest.mark.gpu
def test_prefetch_sampler_reports_an_undersized_expansion():
    """A capacity below the expansion's edge count: GGMS_STATUS_PREFETCH_FULL in the batch's status word, the edge
    count it needed recorded, nothing written past the buffers; the next batch that fits is right again."""
    from xgnn_amd import ops
    from xgnn_amd._lib import GgmsError
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(1)
    N = 3000
    ip, ix = _csr(N, rs, hub=5, hub_deg=20000)
    graph = _device_graph(ip, ix, dev)
    bs = ops.PrefetchBatchSampler(graph, ip, [3, 2], 100, sample_type=ops.KHOP0, seed=2, device=dev,
                                  max_edges_budget=5000)
    seeds = rs.permutation(N)[:100].astype(np.uint32)
    if 5 not in seeds:
        seeds[0] = 5
    bs.sample(torch.from_numpy(seeds.view(np.int32)).to(dev), distinct=True)
    with pytest.raises(GgmsError, match="0x4"):
        bs.result()
    need = int(bs.counts[COUNT_EXPANSION(2)].item())
    assert need == prefetch_replay(oracle.do_sample(oracle.KHOP0, ip, ix, seeds, [3, 2]), ip, ix)["expansion_edges"]
    assert need > 5000
    small = np.array([v for v in range(N) if ip[v + 1] - ip[v] < 3][:20], np.uint32)
    bs.sample(torch.from_numpy(small.view(np.int32)).to(dev), distinct=True)
    got = bs.result()
    want = prefetch_replay(oracle.do_sample(oracle.KHOP0, ip, ix, small, [3, 2]), ip, ix)
    np.testing.assert_array_equal(got["input_nodes"].cpu().numpy().view(np.uint32), want["input_nodes"])


@pytest.mark.gpu
@pytest.mark.parametrize("dim,dtype", [(20, torch.float32), (128, torch.float32), (9, torch.float16)])
def test_dynamic_cache_gather_and_publish(dim, dtype):
    """A sequence of node lists: every gather's bytes equal feat[nodes], its miss count is |cur \\ prev|; the rows of
    hits come from the previous batch's buffer (poisoned host rows would show otherwise).  Across a seq wrap (reset,
    seq 1) nothing hits."""
    from xgnn_amd import ops
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(dim)
    N = 20000
    feat = torch.from_numpy(rs.standard_normal((N, dim)).astype(np.float32)).to(dtype)
    host = feat.to(dev)  # (the engine's runs read the pinned host table; the leaf only needs a second source)
    stamps = torch.empty(N, dtype=torch.int64, device=dev)
    ops.dynamic_cache_reset(stamps)
    seqs = [1, 2, 3, 0xFFFFFFFE, 0xFFFFFFFF, 1, 2]
    prev_nodes, prev_out = None, None
    pool = rs.permutation(N)[:6000]
    for step, seq in enumerate(seqs):
        if step == 5:  # seq wrapped: the table starts again from zero
            ops.dynamic_cache_reset(stamps)
        n = int(rs.randint(500, 5000))
        nodes = rs.choice(pool, n, replace=False).astype(np.uint32)
        nd = torch.from_numpy(nodes.view(np.int32)).to(dev)
        out = torch.full((n, dim), -7, dtype=dtype, device=dev)
        miss = torch.zeros(1, dtype=torch.int64, device=dev)
        ops.extract_dynamic(out, nd, stamps, seq, prev_out, host, num_miss=miss)
        ops.dynamic_cache_publish(stamps, nd, seq)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == feat[torch.from_numpy(nodes.astype(np.int64))].numpy().tobytes(), step
        hits_possible = prev_nodes is not None and seq > 1 and seqs[step - 1] == seq - 1
        want_miss = n - (np.isin(nodes, prev_nodes).sum() if hits_possible else 0)
        assert int(miss.item()) == want_miss, (step, seq)
        prev_nodes, prev_out = nodes, out
    # hits really come from the previous buffer: poison it and re-gather the same list with the next seq
    prev_out.fill_(3)
    out = torch.empty_like(prev_out)
    ops.extract_dynamic(out, torch.from_numpy(prev_nodes.view(np.int32)).to(dev), stamps, seqs[-1] + 1, prev_out, host)
    torch.cuda.synchronize()
    assert (out.float().cpu().numpy() == 3).all()


def _dataset(tmp_path, sample_type):
    from xgnn_amd import datagen
    d = make_dataset(tmp_path)
    if sample_type == "weighted_khop":
        g = dict(indptr=d["ip"], indices=d["ix"], train_set=d["train"], meta=dict(feat_dim=d["feat"].shape[1], num_class=13))
        datagen.write_dataset(d["path"], g, feat=d["feat"], label=d["label"], weights=datagen.edge_weights(g, "default", seed=3))
        d["prob"] = np.fromfile(os.path.join(d["path"], "prob_table.bin"), np.float32)
        d["alias"] = np.fromfile(os.path.join(d["path"], "alias_table.bin"), np.uint32)
    return d


def _replay_batches(d, bs, epochs, fan, seed, sample_type):
    from test_engine import _oracle_batches
    kw = dict(prob=d["prob"], alias=d["alias"]) if sample_type == "weighted_khop" else {}
    want = _oracle_batches(d, 0, 1, bs, epochs, fan, seed, arch6=False, sample_type=sample_type, **kw)
    for w in want.values():
        w["res"] = prefetch_replay(w["res"], d["ip"], d["ix"])
        w["feat"] = oracle.extract(d["feat"], w["res"]["input_nodes"])
    return want


ENGINE = [("khop0", [5, 4], "step"), ("khop1", [4, 3, 2], "start"), ("weighted_khop", [5, 4], "step")]


def _run_engine(tmp_path, d, case, policy, env, tag):
    st, fan, mode = case
    prefix = str(tmp_path / tag)
    args = [f"sample_type={st}", "seed=7", "batch_size=64", "num_epoch=2", "fanout=" + " ".join(map(str, fan)),
            f"cache_policy={policy}", "cache_percentage=0.0"]
    r = subprocess.run([sys.executable, DRIVER4, d["path"], prefix, mode] + args, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(prefix + ".w0.npz"), json.load(open(prefix + ".info.json"))


def _engine_against_replay(tmp_path, case, env):
    from test_engine import _check
    st, fan, _ = case
    d = _dataset(tmp_path / "ds", st)
    want = _replay_batches(d, 64, 2, fan, 7, st)
    row_bytes = d["feat"].shape[1] * 4
    runs = {}
    for policy in ["degree", "dynamic_cache"]:
        npz, info = _run_engine(tmp_path, d, case, policy, env, policy)
        _check(npz, want, len(fan))
        runs[policy] = npz
        prev = None
        for s in info["steps"]:
            w = want[s["key"]]["res"]["input_nodes"]
            assert s["feature_bytes"] == w.size * row_bytes
            assert s["neighbour_s"] > 0 and s["advanced_s"] >= 0
            if policy == "degree":  # every row from host memory
                assert s["miss_bytes"] == w.size * row_bytes, s["key"]
            else:  # rows the previous batch did not have
                nmiss = w.size - (np.isin(w, prev).sum() if prev is not None else 0)
                assert s["miss_bytes"] == nmiss * row_bytes, s["key"]
                assert s["cache_copy_s"] > 0
            prev = w
    a, b = runs["degree"], runs["dynamic_cache"]
    assert a.files == b.files
    for k in a.files:
        if not k.endswith("miss_bytes"):
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENGINE, ids=[f"{c[0]}-{c[2]}" for c in ENGINE])
def test_arch4_forced_equals_the_replay(tmp_path, case):
    """Two epochs under SAMGRAPH_FORCE_DEVICE=0, with and without dynamic_cache: every batch's COO, input nodes,
    features and labels equal the replay, the two runs are byte-identical, kLogL1MissBytes is the replay's."""
    _engine_against_replay(tmp_path, case, FORCED)


@pytest.mark.gpu
@pytest.mark.skipif(not (torch.cuda.is_available() and torch.cuda.device_count() >= 2),
                    reason="fewer than two GPUs visible: arch4's cross-device path is unexercised here")
def test_arch4_two_devices_equals_the_replay(tmp_path):
    """The same on two real GPUs (no SAMGRAPH_FORCE_DEVICE): sampler cuda:1, trainer cuda:0."""
    _engine_against_replay(tmp_path, ENGINE[0], UNFORCED)
