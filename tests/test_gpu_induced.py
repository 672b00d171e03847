"""ggms_induced_edges on the GPU against its numpy statement (tests/induced_ref.py), bit for bit, on hand-built graphs --
no sampler.  Guard words lie around every output array and poison behind M; after every call the membership map is all
EMPTY again, the node list is unchanged, the two count words are exact and the device status is 0.

xgnn_amd/csrc/induced.hip: the owners' lists are walked in edge tiles of TILE = 2048 entries (edge_tiles.h), a lane takes 8
entries 256 apart, a tile stages at most 2048 list heads per round; ranks inside a round come from 64-lane ballots."""
import numpy as np
import pytest

import induced_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WAVE, TILE = 64, 2048
EMPTY = ref.EMPTY
GUARD = 0x5A5A5A5A
POISON = 0x0BADBEEF
GRID_CAP = 3  # GGMS_DEBUG_GRID_CAP


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


# ---- the graph -------------------------------------------------------------------------------------------------------
# node v < len(LENS) has a list of LENS[v] entries; FILL ids are in no test's set, MEM ids are the sets' members, ISO ids
# have no list and are in no list, SHORT ids have lists of 0 and 1 entries alternately
LENS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 17, 40000]
LEN_IDS = ["list0", "list1", "list63", "list64", "list65", "tile-1", "tile", "tile+1", "5tiles+17", "list40000"]
ONE_TILE_HUB, FULL_TILE_HUB = 10, 11  # lists of 5 and 3 tiles (below)
FILL = np.arange(20, 200, dtype=np.uint32)
MEM = np.arange(200, 216, dtype=np.uint32)
ISO = np.arange(220, 230, dtype=np.uint32)
SHORT = np.arange(1000, 3600, dtype=np.uint32)
N = 3700
MEM_DEG = 7
LEAD = MEM.size * MEM_DEG  # list entries in front of an owner that follows all of MEM in a set


def special_offsets(d):
    """Where an owner's list of d entries holds members: its first and last entry and both sides of every tile boundary,
    for an owner that leads its set and for one that follows all of MEM."""
    at = {0, d - 1}
    for b in range(TILE, d + LEAD + 1, TILE):
        at |= {b - 1, b, b - LEAD - 1, b - LEAD}
    return sorted(x for x in at if 0 <= x < d)


@pytest.fixture(scope="module")
def world(ops):
    rng = np.random.RandomState(11)
    deg = np.zeros(N, np.int64)
    deg[:len(LENS)] = LENS
    deg[ONE_TILE_HUB], deg[FULL_TILE_HUB] = 5 * TILE, 3 * TILE
    deg[FILL] = 7
    deg[MEM] = MEM_DEG
    deg[SHORT[1::2]] = 1
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    both = np.concatenate([FILL, MEM])
    ix = both[rng.randint(0, both.size, int(ip[-1]))]
    for v in list(range(len(LENS))) + [ONE_TILE_HUB]:
        ix[ip[v]:ip[v + 1]] = FILL[rng.randint(0, FILL.size, int(deg[v]))]
    for v, d in enumerate(LENS):
        for k, off in enumerate(special_offsets(d)):
            ix[ip[v] + off] = MEM[k % MEM.size]
    ix[ip[3] + 5] = 3  # a self-loop of the 64-entry owner
    ix[ip[MEM[0]]] = MEM[0]  # a member's self-loop
    ix[ip[MEM[1]] + 2:ip[MEM[1]] + 5] = MEM[2]  # three parallel edges
    a = int(ip[ONE_TILE_HUB])
    ix[a + 2 * TILE + 100:a + 2 * TILE + 1900:37] = MEM[3]  # hits in the third tile only
    a = int(ip[FULL_TILE_HUB])
    ix[a:a + TILE] = MEM[rng.randint(0, MEM.size, TILE)]  # a tile of 2048 hits
    ix[a + TILE:a + 2 * TILE] = FILL[rng.randint(0, FILL.size, TILE)]  # a tile of none
    ix[ip[SHORT[1::2]]] = np.where(np.arange(SHORT[1::2].size) % 3 == 0, MEM[5], FILL[0])
    graph = ops.DeviceGraph(dev(ip), dev(ix))
    local_of = ops.induced_map(N)  # ONE map for the whole module: every call must leave it clean
    return ip, ix, graph, local_of


def run_and_check(ops, world, nodes, n=None, cap=None, shift=0, want_eid=True, graph=None, num_edge=None, ipx=None):
    """nodes: the list as the device gets it (max_nodes entries); n: the count on the device (None: no device count).
    cap: max_edges (default: M + 5, so that poison behind M is seen).  shift: row / col / eid start that many words
    behind a 16-byte boundary.  -> the reference's (row, col, eid, M, walked)."""
    ip, ix, g, local_of = world
    if ipx is not None:
        ip, ix = ipx
    g = graph if graph is not None else g
    nodes = np.asarray(nodes, np.uint32)
    live = nodes if n is None else nodes[:n]
    full = ref.induced_edges(ip, ix, live)
    M, walked = full[3], full[4]
    cap = M + 5 if cap is None else cap
    want = ref.induced_edges(ip, ix, live, max_edges=cap)
    keep = min(M, cap)
    bufs = []
    for _ in range(3):
        t = torch.full((shift + cap + 64,), GUARD, dtype=torch.int32, device="cuda")
        t[shift:shift + cap] = POISON
        bufs.append(t)
    out = tuple(t[shift:shift + cap] for t in bufs)
    assert all(t.data_ptr() % 16 == 4 * shift for t in out) or cap == 0
    t_nodes = dev(nodes) if nodes.size else torch.empty(0, dtype=torch.int32, device="cuda")
    t_n = torch.tensor([n], dtype=torch.int64, device="cuda") if n is not None else None
    counts = torch.full((4,), 0x7777, dtype=torch.int64, device="cuda")
    r = ops.induced_edges(g, t_nodes, local_of, cap, num_nodes_dev=t_n, want_eid=want_eid, out=out, counts=counts,
                          num_edge=num_edge if num_edge is not None else len(ix))
    assert r[3] is counts and (r[2] is None) == (not want_eid)
    c = counts.cpu().tolist()
    print(f"{live.size} nodes, M = {M} of {walked} walked, max_edges {cap}; counts {c[:2]}")
    assert c == [M, walked, 0x7777, 0x7777]
    for name, t, w in zip(("row", "col", "eid"), bufs, want[:3]):
        h = host_u32(t)
        assert (h[:shift] == GUARD).all() and (h[shift + cap:] == GUARD).all(), f"{name}: a guard word was written"
        if name == "eid" and not want_eid:
            assert (h[shift:shift + cap] == POISON).all()
            continue
        np.testing.assert_array_equal(h[shift:shift + keep], w, err_msg=name)
        assert (h[shift + keep:shift + cap] == POISON).all(), f"{name}: written behind min(M, max_edges)"
    assert not bool((local_of != -1).any()), "the map is all EMPTY again"
    if nodes.size:
        np.testing.assert_array_equal(host_u32(t_nodes), nodes)
    assert ops.device_status() == 0
    return full


# ---- list lengths x where the members lie ------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(len(LENS)), ids=LEN_IDS)
def test_members_at_the_ends_and_at_every_tile_boundary(ops, world, v):
    """The owner leads its set (its list starts a tile), then follows all of MEM (it starts LEAD entries into one)."""
    ip, ix, _, _ = world
    d = LENS[v]
    for nodes in (np.concatenate([[v], MEM]), np.concatenate([MEM, [v]])):
        row, col, eid, M, walked = run_and_check(ops, world, nodes)
        own = int(np.flatnonzero(nodes == v)[0])
        mine = eid[col == own] - ip[v]
        want = special_offsets(d) + ([5] if v == 3 else [])
        assert sorted(mine.tolist()) == sorted(want) and walked == d + LEAD


@pytest.mark.parametrize("v", range(len(LENS)), ids=LEN_IDS)
def test_members_nowhere(ops, world, v):
    """The owner among nodes that are in no list and have none: M = 0 (but for the one self-loop), everything is walked."""
    full = run_and_check(ops, world, np.concatenate([ISO[:3], [v], ISO[3:]]))
    assert full[3] == (1 if v == 3 else 0) and full[4] == LENS[v]


def test_no_edges_at_all(ops, world):
    assert run_and_check(ops, world, ISO)[3:] == (0, 0)
    assert run_and_check(ops, world, np.concatenate([ISO[:5], [8]]))[3] == 0  # M = 0 behind 5 tiles walked


def test_a_long_run_of_short_lists_in_front_of_a_hub(ops, world):
    """2600 lists of 0 and 1 entries, then the 40000-entry hub: the first tile touches more than 2048 list heads, so its
    staging takes more than one round; then the hub fills the rest of the tile."""
    nodes = np.concatenate([MEM[:6], SHORT, [9], MEM[6:]])
    full = run_and_check(ops, world, nodes)
    assert SHORT.size > TILE and full[4] == 40000 + SHORT.size // 2 + LEAD
    assert (full[1] >= 6).sum() > 400  # the short lists' and the hub's own hits


def test_hits_in_one_tile_only_and_tiles_of_0_and_2048_hits(ops, world):
    ip, ix, _, _ = world
    row, col, eid, M, _ = run_and_check(ops, world, np.concatenate([[ONE_TILE_HUB], MEM]))
    off = eid[col == 0] - ip[ONE_TILE_HUB]
    assert off.size > 40 and (off // TILE == 2).all()
    row, col, eid, M, _ = run_and_check(ops, world, np.concatenate([[FULL_TILE_HUB], MEM]))
    per_tile = np.bincount((eid[col == 0] - ip[FULL_TILE_HUB]) // TILE, minlength=3)
    assert per_tile[0] == TILE and per_tile[1] == 0 and 0 < per_tile[2] < TILE


def test_truncation_keeps_the_canonical_prefix(ops, world):
    nodes = np.concatenate([[8], MEM, [4]])
    M = run_and_check(ops, world, nodes)[3]
    assert M > 20
    for cap in (M, M - 1, 1, 0):
        assert run_and_check(ops, world, nodes, cap=cap)[3] == M  # the count says what exists


def test_no_nodes(ops, world):
    assert run_and_check(ops, world, np.zeros(0, np.uint32))[3:] == (0, 0)  # max_nodes = 0
    assert run_and_check(ops, world, np.concatenate([[9], MEM]), n=0)[3:] == (0, 0)  # n = 0 on the device


def test_device_count_below_max_nodes(ops, world):
    """What lies behind n is not part of the set: a hub, members, garbage."""
    live = np.concatenate([[7], MEM[:9]])
    nodes = np.concatenate([live, [9], MEM[9:], [0x7FFFFFFF, EMPTY, N]]).astype(np.uint32)
    full = run_and_check(ops, world, nodes, n=live.size)
    assert full[4] == LENS[7] + 9 * MEM_DEG


def test_repeated_ids(ops, world):
    """The hub three times (its first position owns), a member's copies, and a repeat as the last entry."""
    nodes = np.concatenate([MEM[:4], [9], MEM[4:], [9], MEM[2:5], [9, 6], MEM[3:4]]).astype(np.uint32)
    row, col, eid, M, walked = run_and_check(ops, world, nodes)
    assert walked == 40000 + LENS[6] + LEAD and set(col.tolist()) <= set(range(MEM.size + 1)) | {nodes.size - 2}
    assert row.max() <= MEM.size + 1  # targets map to first positions


def test_ids_that_are_no_node(ops, world):
    nodes = np.concatenate([[EMPTY, N, 5], MEM[:8], [N + 77, 0xFFFFFFFE, EMPTY], MEM[8:], [EMPTY]]).astype(np.uint32)
    full = run_and_check(ops, world, nodes)
    assert full[4] == LENS[5] + LEAD


def test_self_loops_and_parallel_edges(ops, world):
    ip, ix, _, _ = world
    row, col, eid, M, _ = run_and_check(ops, world, np.concatenate([MEM, [3]]))
    assert ((row == col) & (col == 0)).any() and ((row == col) & (col == MEM.size)).any()  # MEM[0]'s and node 3's
    par = eid[(col == 1) & (row == 2)]
    assert par.size >= 3 and np.unique(par).size == par.size  # each copy under its own position


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_caps(ops, world, cap):
    """One and three workgroups for every launch: every tile loop goes round many times."""
    from xgnn_amd._lib import lib
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        run_and_check(ops, world, np.concatenate([MEM[:3], SHORT[:700], [9, 8], MEM[3:], [FULL_TILE_HUB]]))
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_outputs_off_a_16_byte_boundary(ops, world, shift):
    run_and_check(ops, world, np.concatenate([[8], MEM, [FULL_TILE_HUB]]), shift=shift)


def test_without_eid(ops, world):
    run_and_check(ops, world, np.concatenate([[8], MEM, [3]]), want_eid=False)


def test_two_shard_view_equals_the_whole_csr(ops, world):
    import oracle
    ip, ix, _, local_of = world
    P, ncn = 2, 2000  # the owners and members in shards, most SHORT nodes in the whole CSR of slot P
    parts = [oracle.partition_graph(ip, ix, r, P, ncn) for r in range(P)]
    g = ops.DeviceGraph(None, None, part_indptr=[dev(p[0]) for p in parts] + [dev(ip)],
                        part_indices=[dev(p[1]) for p in parts] + [dev(ix)], num_cache_node=ncn)
    nodes = np.concatenate([MEM[:5], SHORT[::3], [9, 4], MEM[5:]]).astype(np.uint32)
    run_and_check(ops, world, nodes, graph=g, want_eid=False)
    with pytest.raises(Exception, match="sharded"):
        ops.induced_edges(g, dev(nodes), local_of, 10, num_edge=len(ix))


def test_positions_past_2_31(ops, world):
    """The hub's list lies across edge position 2^31: eid there no longer fits a signed 32-bit integer."""
    from graphgen import high_offset_csr
    from test_gpu_high_offset_graph import seeds_of
    g = high_offset_csr(1 << 31, seed=31)
    graph = ops.DeviceGraph(dev(g.indptr), g.indices)
    local_of = ops.induced_map(g.indptr.size - 1)
    nodes = seeds_of(g, 301, np.random.RandomState(31))
    full = run_and_check(ops, (g.indptr, g.ix, graph, local_of), nodes, num_edge=g.num_edge)
    assert (full[2] >= 1 << 31).any() and (full[2] < 1 << 30).any() and full[3] > 100
    del graph, g
    torch.cuda.empty_cache()


def test_two_calls_on_one_map_with_different_sets(ops, world):
    """The second call must not see the first's marks: MEM is in the first set only."""
    a = run_and_check(ops, world, np.concatenate([[8], MEM]))
    b = run_and_check(ops, world, np.concatenate([[8], FILL[:16]]))
    assert a[3] > 0 and not np.array_equal(a[0], b[0])
