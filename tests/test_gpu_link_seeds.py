"""ggms_link_seeds on the GPU against its numpy statement (tests/link_ref.py), bit for bit: every list length at which
the wave's chunked walk changes shape, a hub of several chunk groups, multi-edges, a self-loop, runs of empty rows,
forced negatives, the NULL forced counter, the exclusion property on the GPU's own output, and edge ids out of range."""
import ctypes as C

import numpy as np
import pytest

import link_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# xgnn_amd/csrc/link_seeds.hip walks a source's list in groups of kLinkWide x 64 = 2048 ids while that many are left,
# then in groups of kLinkChunks x 64 = 512 ids (the last one partial)
GROUP, WIDE = 512, 2048
LONG = {30: WIDE - 1, 31: WIDE, 32: WIDE + 1, 33: 2 * WIDE + GROUP + 92}  # rows around the wide walk's threshold
N = 1500
HUB = 700  # the node whose list has 1100 entries: three groups, the last one partial


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
def big(ops):
    """1500 nodes.  Rows 0 .. 4, 600 .. 609 and 1490 .. 1499 are empty; rows 10 .. 17 have 0, 1, 63, 64, 65, 128, 129
    and 257 entries, row 20 is one id repeated 70 times with others between (multi-edges), row 21 holds itself, rows
    30 .. 33 have 2047, 2048, 2049 and 4700 entries (the wide walk: none, exactly one group, one group and a one-id
    tail, two groups and two tail groups), row HUB has 1100 entries; every other row 0 .. 40."""
    rng = np.random.RandomState(15)
    deg = rng.randint(0, 41, N)
    deg[:5] = deg[600:610] = deg[1490:] = 0
    deg[10:18] = [0, 1, 63, 64, 65, 128, 129, 257]
    deg[HUB] = 1100
    for v, d in LONG.items():
        deg[v] = d
    lists = [rng.randint(0, N, d) for d in deg]
    lists[20] = np.concatenate([np.full(35, 33), rng.randint(0, N, 10), np.full(35, 33)])
    lists[21] = np.array([5, 21, 900])
    ip, ix = ref.graph_of_lists(lists)
    return ip, ix, ops.DeviceGraph(dev(ip), dev(ix))


def edge_ids_of(ip, B):
    """Edge 0 and E - 1, the boundaries of the special rows and of the hub, repeated ids, then random ones."""
    E = int(ip[-1])
    if B == 1:
        return np.array([int(ip[HUB]) + 600], np.uint32)
    if B == 3:
        return np.array([0, E - 1, int(ip[HUB])], np.uint32)
    rows = list(range(11, 18)) + [20, 21, HUB, 5, 599, 610, 1489] + sorted(LONG)
    ids = [0, E - 1]
    for v in rows:
        if ip[v + 1] > ip[v]:
            ids += [int(ip[v]), int(ip[v + 1]) - 1]
    ids += [int(ip[HUB]) + GROUP - 1, int(ip[HUB]) + GROUP, int(ip[HUB]) + 2 * GROUP, 0, 0, E - 1, int(ip[HUB]),
            int(ip[33]) + WIDE - 1, int(ip[33]) + WIDE, int(ip[33]) + 2 * WIDE]
    rng = np.random.RandomState(B)
    ids += rng.randint(0, E, B - len(ids)).tolist()
    assert len(ids) == B
    return np.array(ids, np.uint32)


_want = {}


def want_of(ip, ix, eids, K, mode, salt, tag):
    if tag not in _want:  # one reference per case, shared by the tests that need it
        _want[tag] = ref.link_seeds(ip, ix, eids, K, mode, salt)
    return _want[tag]


@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("mode", [ref.UNIFORM, ref.EXCLUDE], ids=["uniform", "exclude"])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_equals_the_reference(ops, big, K, mode, B):
    ip, ix, g = big
    eids = edge_ids_of(ip, B)
    salt = 0xA5000000 + 131 * K + B
    out, forced = ops.link_seeds(g, dev(eids), K, mode, salt)
    want, want_forced = want_of(ip, ix, eids, K, mode, salt, (K, mode, B))
    got = host_u32(out)
    assert got.size == B * (2 + K)
    src, dst, neg = ref.split(got, K)
    wsrc, wdst, wneg = ref.split(want, K)
    np.testing.assert_array_equal(src, wsrc)
    np.testing.assert_array_equal(dst, wdst)
    np.testing.assert_array_equal(neg, wneg)
    print(f"K {K} mode {mode} B {B}: forced {int(forced.item())}")
    assert int(forced.item()) == want_forced
    assert ops.device_status() == 0
    # NULL forced counter: the same outputs
    out2, none = ops.link_seeds(g, dev(eids), K, mode, salt, count_forced=False)
    assert none is None
    np.testing.assert_array_equal(host_u32(out2), got)


def test_hub_rejects_retries_and_forces(ops, big):
    """Every edge of the hub's list as a positive (1100 / 1500 of the candidates are its neighbours): the three outcomes
    all occur, as the reference decides."""
    ip, ix, g = big
    eids = np.arange(int(ip[HUB]), int(ip[HUB]) + 200, dtype=np.uint32)
    out, forced = ops.link_seeds(g, dev(eids), 5, ref.EXCLUDE, 3)
    want, want_forced = ref.link_seeds(ip, ix, eids, 5, ref.EXCLUDE, 3)
    np.testing.assert_array_equal(host_u32(out), want)
    first = ref.link_seeds(ip, ix, eids, 5, ref.UNIFORM, 3)[0]
    kept = int((ref.split(want, 5)[2] == ref.split(first, 5)[2]).sum())
    assert int(forced.item()) == want_forced and 0 < want_forced < 1000 and 0 < kept < 1000 - want_forced


def test_exclusion_property_of_the_output_itself(ops, big):
    """Mode exclude, no reference: a negative is the source or one of its neighbours only if it was forced, so the
    banned negatives are exactly as many as the device counted."""
    ip, ix, g = big
    E = int(ip[-1])
    eids = np.random.RandomState(8).randint(0, E, 400).astype(np.uint32)
    eids[:50] = np.arange(int(ip[HUB]), int(ip[HUB]) + 50)
    K = 7
    out, forced = ops.link_seeds(g, dev(eids), K, ref.EXCLUDE, 0x51)
    src, dst, neg = ref.split(host_u32(out), K)
    banned = 0
    for i, e in enumerate(eids.tolist()):
        u = int(src[i])
        assert ip[u] <= e < ip[u + 1] and dst[i] == ix[e]
        row = set(ix[ip[u]:ip[u + 1]].tolist()) | {u}
        banned += sum(int(w) in row for w in neg[i])
    assert (neg < N).all() and banned == int(forced.item())


def test_complete_graph_forces_everything(ops):
    ip, ix = ref.complete_graph(8)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    for B, K in [(1, 1), (3, 5), (257, 64)]:
        eids = np.random.RandomState(B).randint(0, 56, B).astype(np.uint32)
        out, forced = ops.link_seeds(g, dev(eids), K, ref.EXCLUDE, 11)
        want, want_forced = ref.link_seeds(ip, ix, eids, K, ref.EXCLUDE, 11)
        np.testing.assert_array_equal(host_u32(out), want)
        assert int(forced.item()) == want_forced == B * K


def test_source_adjacent_to_all_but_two(ops):
    """16 nodes, node 3 adjacent to every node but 6 and 11 (itself included): a candidate is accepted with probability
    1 / 8, so accepted, retried and forced negatives all occur."""
    lists = [[(v + 1) % 16] for v in range(16)]
    lists[3] = [w for w in range(16) if w not in (6, 11)]
    ip, ix = ref.graph_of_lists(lists)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    eids = np.arange(int(ip[3]), int(ip[4]), dtype=np.uint32)
    K = 64
    out, forced = ops.link_seeds(g, dev(eids), K, ref.EXCLUDE, 2024)
    want, want_forced = ref.link_seeds(ip, ix, eids, K, ref.EXCLUDE, 2024)
    np.testing.assert_array_equal(host_u32(out), want)
    neg = ref.split(want, K)[2]
    first = ref.split(ref.link_seeds(ip, ix, eids, K, ref.UNIFORM, 2024)[0], K)[2]
    ok = np.isin(neg, [6, 11])
    assert int(forced.item()) == want_forced == int((~ok).sum())
    assert want_forced > 0 and (ok & (neg == first)).sum() > 0 and (ok & (neg != first)).sum() > 0


def test_edge_ids_out_of_range(ops, big):
    """An id >= E leaves GGMS_EMPTY_KEY in its positive's 2 + K positions; every other position is what it is without
    the bad ids, and nothing outside the B (2 + K) entries is written."""
    from xgnn_amd._lib import check, lib
    ip, ix, g = big
    E = int(ip[-1])
    K, salt = 5, 77
    eids = edge_ids_of(ip, 257).copy()
    bad = [0, 100, 256]
    eids[bad] = [E, E + 12345, 0xFFFFFFFF]
    B = eids.size
    GUARD = 0x5A5A5A5A
    out = torch.full((B * (2 + K) + 64,), GUARD, dtype=torch.int32, device="cuda")
    forced = torch.zeros(1, dtype=torch.int64, device="cuda")
    t = dev(eids)
    check(lib().ggms_link_seeds(C.byref(g.c), C.c_void_p(t.data_ptr()), B, K, ref.EXCLUDE, salt,
                                C.c_void_p(out.data_ptr()), C.c_void_p(forced.data_ptr()),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ggms_link_seeds")
    got = host_u32(out)
    assert (got[B * (2 + K):] == GUARD).all()
    want, want_forced = ref.link_seeds(ip, ix, eids, K, ref.EXCLUDE, salt)
    np.testing.assert_array_equal(got[:B * (2 + K)], want)
    src, dst, neg = ref.split(got[:B * (2 + K)], K)
    assert (src[bad] == ref.EMPTY).all() and (dst[bad] == ref.EMPTY).all() and (neg[bad] == ref.EMPTY).all()
    good = np.setdiff1d(np.arange(B), bad)
    clean = ref.split(want_of(ip, ix, edge_ids_of(ip, 257), K, ref.EXCLUDE, salt, "clean-257")[0], K)
    assert (src[good] == clean[0][good]).all() and (neg[good] == clean[2][good]).all() and (neg[good] != ref.EMPTY).all()
    assert int(forced.item()) == want_forced and ops.device_status() == 0


def test_keyed_by_the_edge_id_and_empty_call(ops, big):
    ip, ix, g = big
    eids = edge_ids_of(ip, 257)
    a = ref.split(host_u32(ops.link_seeds(g, dev(eids), 5, ref.EXCLUDE, 9)[0]), 5)[2]
    perm = np.random.RandomState(0).permutation(257)
    b = ref.split(host_u32(ops.link_seeds(g, dev(eids[perm]), 5, ref.EXCLUDE, 9)[0]), 5)[2]
    np.testing.assert_array_equal(b, a[perm])
    out, forced = ops.link_seeds(g, torch.zeros(0, dtype=torch.int32, device="cuda"), 5, ref.EXCLUDE, 9)
    assert out.numel() == 0 and int(forced.item()) == 0
