"""presample_static on the GPU: the L-hop closure operator (ggms_khop_closure) against a numpy BFS, and the cache
ranking it makes inside the engine (arch3, arch5, arch6) against a numpy replay of the ranking."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from graphgen import hub_csr, powerlaw_csr
from test_engine import DRIVER, _check, _oracle_batches, make_dataset
from test_gpu_arch3 import DRIVER3, FORCED
from test_gpu_arch5 import DRIVER5, _oracle_arch5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as o
    return o


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def bfs_levels(ip, ix, seeds, num_hop):
    """Nodes at distance exactly h = 0 .. num_hop from the seeds, each level sorted."""
    N = ip.size - 1
    seen = np.zeros(N, bool)
    cur = np.unique(np.asarray(seeds, np.uint32))
    seen[cur] = True
    levels = [cur]
    for _ in range(num_hop):
        starts, lens = ip[cur].astype(np.int64), (ip[cur + 1] - ip[cur]).astype(np.int64)
        total = int(lens.sum())
        pos = np.repeat(starts - np.cumsum(lens) + lens, lens) + np.arange(total, dtype=np.int64)
        nb = np.unique(ix[pos]) if total else np.zeros(0, np.uint32)
        nb = nb[~seen[nb]]
        seen[nb] = True
        levels.append(nb.astype(np.uint32))
        cur = nb
    return levels


def _closure_levels(ops, g, seeds, num_hop, visit, stamp, freq=None):
    c, off = ops.khop_closure(g, _dev(seeds), num_hop, visit, stamp, freq)
    c, off = c.cpu().numpy().view(np.uint32), off.cpu().numpy()
    assert off.size == num_hop + 2 and off[0] == 0 and off[-1] == c.size and np.all(np.diff(off) >= 0)
    return [np.sort(c[off[h]:off[h + 1]]) for h in range(num_hop + 1)]


def _big_hub_csr():
    """One hub of 250 000 neighbours among short lists, plus zero-degree nodes."""
    rng = np.random.RandomState(4)
    N = 60_000
    deg = rng.randint(0, 6, N).astype(np.int64)
    deg[123] = 250_000
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    return ip, rng.randint(0, N, int(ip[-1])).astype(np.uint32)


def _loops_and_multi_csr():
    """Self loops and parallel edges on every list."""
    rng = np.random.RandomState(8)
    N = 5000
    lists = []
    for v in range(N):
        nb = list(rng.randint(0, N, rng.randint(0, 5)))
        nb += [v] * rng.randint(0, 3)  # self loops
        nb += nb[:2]                   # parallel edges
        lists.append(np.array(nb, np.uint32))
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum([x.size for x in lists])
    return ip, np.concatenate(lists).astype(np.uint32)


GRAPHS = {
    "powerlaw": lambda: powerlaw_csr(20_000, mean_deg=8, seed=3),
    "hub": lambda: hub_csr(),
    "big_hub": _big_hub_csr,
    "loops_multi": _loops_and_multi_csr,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_closure_levels_equal_bfs(ops, name):
    """Every hop segment, sorted, is the BFS level; duplicate seeds, no seeds and a seed without neighbours included;
    one visit array across all calls, a new stamp per call."""
    ip, ix = GRAPHS[name]()
    N = ip.size - 1
    g = ops.DeviceGraph(_dev(ip), _dev(ix))
    deg = np.diff(ip.astype(np.int64))
    rng = np.random.RandomState(1)
    isolated = np.flatnonzero(deg == 0)[:1]
    hubs = np.argsort(deg)[-2:]
    inputs = [rng.randint(0, N, 300), np.concatenate([rng.randint(0, N, 50)] * 3), np.zeros(0, np.uint32),
              np.concatenate([isolated, rng.randint(0, N, 5)]), hubs, rng.randint(0, N, 5000)]
    visit = torch.zeros(N, dtype=torch.int32, device="cuda")
    stamp = 0
    for seeds in inputs:
        for L in range(4):
            stamp += 1
            got = _closure_levels(ops, g, seeds, L, visit, stamp)
            want = bfs_levels(ip, ix, seeds, L)
            for h in range(L + 1):
                np.testing.assert_array_equal(got[h], want[h], err_msg=f"{name} L={L} hop {h} seeds {seeds.size}")
    ops.check_device_status("khop_closure")


@pytest.mark.gpu
def test_closure_freq_counts_each_node_once_per_call(ops):
    """Two calls with stamps 1 and 2 on one visit / freq pair: freq = 2 exactly on the overlap of the two closures."""
    ip, ix = powerlaw_csr(20_000, mean_deg=6, seed=5)
    N = ip.size - 1
    g = ops.DeviceGraph(_dev(ip), _dev(ix))
    visit = torch.zeros(N, dtype=torch.int32, device="cuda")
    freq = torch.zeros(N, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(2)
    a, b = rng.randint(0, N, 400), rng.randint(0, N, 400)
    ca = np.concatenate(_closure_levels(ops, g, a, 2, visit, 1, freq))
    cb = np.concatenate(_closure_levels(ops, g, b, 2, visit, 2, freq))
    want = np.zeros(N, np.int64)
    want[ca] += 1
    want[cb] += 1
    np.testing.assert_array_equal(freq.cpu().numpy(), want)
    assert (want == 2).sum() == np.intersect1d(ca, cb).size > 0
    ops.check_device_status("khop_closure freq")


def _sparse_lists_csr():
    """Every 50th of 8000 nodes has a list of 20 neighbours, the rest have none."""
    N = 8000
    deg = np.zeros(N, np.int64)
    deg[::50] = 20
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    return ip, np.random.RandomState(6).randint(0, N, int(ip[-1])).astype(np.uint32)


@pytest.mark.gpu
def test_closure_frontier_with_long_runs_of_empty_lists(ops):
    """A frontier of 6000 nodes of which every 50th has a list: between two lists of one edge tile lie more frontier
    nodes than the walk stages at once, so a tile takes several rounds.  Levels equal the BFS, freq counts each closure
    node once."""
    ip, ix = _sparse_lists_csr()
    N = ip.size - 1
    seeds = np.arange(6000, dtype=np.uint32)
    want = bfs_levels(ip, ix, seeds, 2)
    assert want[0].size == 6000 and want[1].size > 0  # the hop-0 frontier is expanded into something new
    g = ops.DeviceGraph(_dev(ip), _dev(ix))
    visit = torch.zeros(N, dtype=torch.int32, device="cuda")
    freq = torch.zeros(N, dtype=torch.int32, device="cuda")
    got = _closure_levels(ops, g, seeds, 2, visit, 1, freq)
    for h in range(3):
        np.testing.assert_array_equal(got[h], want[h], err_msg=f"hop {h}")
    want_freq = np.zeros(N, np.int64)
    want_freq[np.concatenate(want)] = 1
    np.testing.assert_array_equal(freq.cpu().numpy(), want_freq)
    ops.check_device_status("khop_closure empty runs")


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3])
def test_closure_through_topology_shards(ops, P):
    """A sharded view (nodes below num_cache_node in P shards, the rest in the whole CSR of the host slot, registered
    host memory) gives the sets of the plain CSR."""
    from xgnn_amd import ggms_store
    ip, ix = GRAPHS["hub"]()
    N = ip.size - 1
    ncn = ggms_store.num_cache_node_for(ip, 0.5)
    assert 0 < ncn < N
    t_ip, t_ix = _dev(ip), _dev(ix)
    pip, pix = ggms_store.topology_shards(t_ip, t_ix, P, ncn)
    host_ix = ops.RegisteredHost(ix.view(np.int32))
    try:
        g = ops.DeviceGraph(None, None, part_indptr=pip + [t_ip], part_indices=pix + [host_ix.tensor],
                            num_cache_node=ncn)
        plain = ops.DeviceGraph(t_ip, t_ix)
        v1 = torch.zeros(N, dtype=torch.int32, device="cuda")
        v2 = torch.zeros(N, dtype=torch.int32, device="cuda")
        rng = np.random.RandomState(P)
        for k, seeds in enumerate([rng.randint(0, N, 200), rng.randint(0, N, 17), np.arange(ncn - 3, ncn + 3)]):
            got = _closure_levels(ops, g, seeds, 3, v1, k + 1)
            ref = _closure_levels(ops, plain, seeds, 3, v2, k + 1)
            want = bfs_levels(ip, ix, seeds, 3)
            for h in range(4):
                np.testing.assert_array_equal(got[h], want[h])
                np.testing.assert_array_equal(ref[h], want[h])
        torch.cuda.synchronize()
        ops.check_device_status("khop_closure shards")
    finally:
        # this process goes on: the registration must not outlive the pages it pins (a later allocation at the same
        # address would be taken for registered memory by the runtime's copies)
        torch.cuda.synchronize()
        g = None
        host_ix.close()


def static_rank(d, seed, bs, fan, epochs):
    """The presample_static ranking: per epoch the engine's presample shuffle, per batch its L-hop closure, +1 per
    closure node; (freq << 32 | id) descending."""
    N = d["ip"].size - 1
    freq = np.zeros(N, np.uint64)
    train = d["train"].copy()
    for e in range(epochs):
        train = oracle.shuffle_minstd0(train, seed + 0x5A5A5A + e)
        for off in range(0, train.size, bs):
            freq[np.concatenate(bfs_levels(d["ip"], d["ix"], train[off:off + bs], len(fan)))] += 1
    keys = (freq << np.uint64(32)) | np.arange(N, dtype=np.uint64)
    return (np.sort(keys)[::-1] & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _check_misses(npz, want, rank, ratio, row_bytes, keys=None):
    N = rank.size
    cached = np.zeros(N, bool)
    cached[rank[: int(N * ratio)]] = True
    for key in (keys if keys is not None else want):
        nmiss = int((~cached[want[key]["res"]["input_nodes"]]).sum())
        assert float(npz[f"{key}:miss_bytes"]) == nmiss * row_bytes, key


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "start"])
def test_arch3_presample_static(tmp_path, mode):
    """arch3: the batches of three epochs are those of a run without presample (no RNG state consumed, the training
    shuffler untouched); the misses are the input nodes outside the cached prefix of the static ranking."""
    d = make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    seed, bs, epochs, fan, ratio = 7, 64, 3, [5, 4], 0.4
    r = subprocess.run([sys.executable, DRIVER3, d["path"], prefix, mode, "sample_type=khop3", f"seed={seed}",
                        f"batch_size={bs}", f"num_epoch={epochs}", "fanout=5 4", f"cache_percentage={ratio}",
                        "cache_policy=presample_static", "presample_epoch=2"],
                       capture_output=True, text=True, timeout=600, env=FORCED)
    assert r.returncode == 0, r.stderr[-3000:]
    want = _oracle_batches(d, 0, 1, bs, epochs, fan, seed, arch6=False)
    npz = np.load(prefix + ".w0.npz")
    _check(npz, want, len(fan))
    _check_misses(npz, want, static_rank(d, seed, bs, fan, 2), ratio, d["feat"].shape[1] * 4)


@pytest.mark.gpu
@pytest.mark.parametrize("dist_graph", [False, True])
def test_arch6_presample_static(tmp_path, dist_graph):
    """arch6, two workers with a partitioned cache: worker 0 ranks by closures (through the sharded view with
    use_dist_graph), both workers' caches hold the ranking's prefix, and the batches are the plain replay's."""
    d = make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    env = dict(os.environ, SAMGRAPH_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    seed, bs, fan, ratio = 17, 64, [5, 4], 0.3
    extra = ["use_dist_graph=0.5"] if dist_graph else []
    r = subprocess.run([sys.executable, DRIVER, d["path"], prefix, "arch6", "2", f"seed={seed}", f"batch_size={bs}",
                        "fanout=5 4", "cache_policy=presample_static", "presample_epoch=2", f"cache_percentage={ratio}",
                        "part_cache=True", "gpu_extract=True"] + extra,
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    rank = static_rank(d, seed, bs, fan, 2)
    for w in range(2):
        want = _oracle_batches(d, w, 2, bs, 2, fan, seed, arch6=True)
        npz = np.load(f"{prefix}.w{w}.npz")
        _check(npz, want, 2)
        _check_misses(npz, want, rank, ratio, d["feat"].shape[1] * 4)


@pytest.mark.gpu
def test_arch5_presample_static(tmp_path):
    """arch5, 2 samplers + 2 trainers: sampler 0 ranks by closures and publishes; every trainer's cache is the
    ranking's prefix and every batch is the plain replay's."""
    d = make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    S, T, seed, bs, epochs, fan, ratio = 2, 2, 7, 48, 2, [5, 4], 0.4
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER5, d["path"], prefix, str(S), str(T), "start",
                        "sample_type=khop3", f"seed={seed}", f"batch_size={bs}", f"num_epoch={epochs}", "fanout=5 4",
                        f"cache_percentage={ratio}", "cache_policy=presample_static", "presample_epoch=1",
                        "queue_timeout_s=60", "barrier_timeout=120"],
                       capture_output=True, text=True, timeout=300, env=FORCED)
    assert r.returncode == 0, r.stderr[-3000:]
    want = _oracle_arch5(d, S, bs, epochs, fan, seed, "khop3", None)
    rank = static_rank(d, seed, bs, fan, 1)
    seen = []
    for w in range(T):
        npz = np.load(f"{prefix}.t{w}.npz")
        mine = sorted({int(k.split(":")[0]) for k in npz.files})
        _check(npz, {k: want[k] for k in mine}, len(fan))
        _check_misses(npz, want, rank, ratio, d["feat"].shape[1] * 4, mine)
        seen += mine
    assert sorted(seen) == sorted(want)
