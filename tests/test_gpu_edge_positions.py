"""ggms_edge_positions on the GPU against its numpy statement (tests/edge_positions_ref.py), bit for bit, on hand-built
layers -- no sampler.  Guard words lie around every eid array and poison behind n_i; the device status stays 0.

xgnn_amd/csrc/edge_positions.hip: a workgroup takes UNIT = 256 consecutive edges of a layer per round, each of its four
waves a CHUNK of 64; a wave walks the runs of equal col among its lanes and streams each run's list in 64-entry pieces.
Lists longer than LONG = 1024 entries are queued per chunk and walked by the second kernel, PARTS = 4 workgroups (16
waves) per queued chunk, combined with a minimum."""
import ctypes as C

import numpy as np
import pytest

import edge_positions_ref as ref
import graphgen

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHUNK, UNIT, LONG, PARTS = 64, 256, 1024, 4
EMPTY = ref.EMPTY
GUARD = 0x5A5A5A5A
POISON = 0x0BADBEEF
INVALID = -1
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


def run_and_check(ops, g, ip, ix, layers, id_map=None, shift=0, num_edge=None):
    """layers: [(row, col, n, max_edges)] -- row / col hold max_edges entries, the first n are the layer (what lies behind
    is poison).  shift: row / col / eid start that many words behind a 16-byte boundary.  -> the reference's positions."""
    from xgnn_amd import _lib
    L = len(layers)
    counts = np.arange(7000, 7000 + _lib.COUNTS_WORDS(L), dtype=np.int64)
    bufs, eid_bufs = [], []
    for i, (row, col, n, cap) in enumerate(layers):
        assert row.size == col.size == cap and n <= cap
        counts[_lib.COUNT_EDGES(i)] = n
        pair = []
        for a in (row, col):
            t = torch.full((shift + cap + 64,), GUARD, dtype=torch.int32, device="cuda")
            t[shift:shift + cap] = dev(a)
            pair.append(t)
        bufs.append(pair)
        e = torch.full((shift + cap + 64,), GUARD, dtype=torch.int32, device="cuda")
        e[shift:shift + cap] = POISON
        eid_bufs.append(e)
    caps = [cap for *_, cap in layers]
    rows = [r[shift:shift + cap] for (r, _), cap in zip(bufs, caps)]
    cols = [c[shift:shift + cap] for (_, c), cap in zip(bufs, caps)]
    eids = [e[shift:shift + cap] for e, cap in zip(eid_bufs, caps)]
    assert all(t.data_ptr() % 16 == 4 * shift for t in rows + cols + eids)
    t_counts = torch.from_numpy(counts.copy()).cuda()
    t_map = dev(id_map) if id_map is not None else None
    got = ops.edge_positions(g, rows, cols, t_counts, id_map=t_map, max_edges=caps, eids=eids, num_edge=num_edge)
    assert got is eids
    want = ref.edge_positions(ip, ix, [row[:n] for row, _, n, _ in layers], [col[:n] for _, col, n, _ in layers], id_map)
    np.testing.assert_array_equal(t_counts.cpu().numpy(), counts)  # no counts word is written
    for i, (e, (row, col, n, cap)) in enumerate(zip(eid_bufs, layers)):
        h = host_u32(e)
        print(f"layer {i}: {n} edges of {cap}, {int((want[i] == EMPTY).sum())} without a position")
        np.testing.assert_array_equal(h[shift:shift + n], want[i], err_msg=f"eid of layer {i}")
        assert (h[shift + n:shift + cap] == POISON).all(), "entries behind n_i are not written"
        assert (h[:shift] == GUARD).all() and (h[shift + cap:] == GUARD).all()
        np.testing.assert_array_equal(host_u32(bufs[i][0])[shift:shift + cap], row)  # row / col are read only
        np.testing.assert_array_equal(host_u32(bufs[i][1])[shift:shift + cap], col)
    assert ops.device_status() == 0
    return want


# ---- a graph whose node v has a list of LENS[v] entries ---------------------------------------------------------------
LENS = [0, 1, 63, 64, 65, LONG - 1, LONG, LONG + 1, 5 * LONG + 17, 40000]
LEN_IDS = ["list0", "list1", "list63", "list64", "list65", "list_long-1", "list_long", "list_long+1", "list_5long",
           "list_40000"]
N = 400  # nodes; ids N - 1 (in no list) and N - 2 (the LAST entry of every list of 2 or more, nowhere else)
ABSENT, LAST = N - 1, N - 2


@pytest.fixture(scope="module")
def ladder(ops):
    rng = np.random.RandomState(5)
    deg = np.full(N, 7, np.int64)
    deg[:len(LENS)] = LENS
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, N - 2, int(ip[-1])).astype(np.uint32)  # lists longer than N hold repeated ids
    for v in range(N):
        if deg[v] >= 2:
            ix[ip[v + 1] - 1] = LAST
    return ip, ix, ops.DeviceGraph(dev(ip), dev(ix))


def run_of(ip, ix, s, m, rng):
    """m edges of seed s: its first and last entry, an absent id, then entries at random positions (repeats included)."""
    a, b = int(ip[s]), int(ip[s + 1])
    t = np.full(m, ABSENT, np.uint32)
    if b > a:
        t[:] = ix[rng.randint(a, b, m)]
        t[0] = ix[a]
        if m > 1:
            t[1] = ix[b - 1]
        if m > 2:
            t[2] = ABSENT
        if m > 4:
            t[4] = t[3]  # a repeated target
    return t, np.full(m, s, np.uint32)


def layer_of(ip, ix, runs, seed=0):
    rng = np.random.RandomState(seed)
    parts = [run_of(ip, ix, s, m, rng) for s, m in runs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


RUNS = [1, 63, 64, 65, 300]  # 300: cut by two chunk boundaries and, at these offsets, by a workgroup's unit


@pytest.mark.parametrize("v", range(len(LENS)), ids=LEN_IDS)
def test_runs_of_1_63_64_65_and_a_cut_run_on_every_list_length(ops, ladder, v):
    ip, ix, g = ladder
    # the runs of node v, a short node's edges between them (or equal neighbours would merge into one run)
    runs = []
    for m in RUNS:
        runs += [(v, m), (20 + m % 7, 3)]
    row, col = layer_of(ip, ix, runs, seed=v)
    n = row.size
    want = run_and_check(ops, g, ip, ix, [(row, col, n, n)])[0]
    at = 1 + 3 + 63 + 3 + 64 + 3  # the run of 65: first entry, last entry, absent
    if LENS[v] >= 1:
        assert want[at] == ip[v] and want[at + 1] == ip[v + 1] - 1 and want[at + 2] == EMPTY
    else:
        assert (want[at:at + 65] == EMPTY).all()
    found = want[want != EMPTY]
    assert (ix[found] == row[want != EMPTY]).all()


def test_first_copy_of_repeated_ids_and_repeated_targets(ops):
    """One list with every id three times: all copies' targets get the first copy's position."""
    ix = np.tile(np.arange(50, dtype=np.uint32), 3)
    ip = np.zeros(151, np.uint32)
    ip[1:] = 150
    g = ops.DeviceGraph(dev(ip), dev(ix))
    row = np.tile(np.arange(50, dtype=np.uint32), 4)
    col = np.zeros(200, np.uint32)
    want = run_and_check(ops, g, ip, ix, [(row, col, 200, 200)])[0]
    np.testing.assert_array_equal(want, row)


def test_hub_targets_at_the_first_and_last_position_and_absent(ops):
    ip, ix = graphgen.hub_csr()
    ix = ix.copy()
    n_node = ip.size - 1
    hubs = np.flatnonzero(np.diff(ip.astype(np.int64)) > LONG)
    assert hubs.size >= 4
    absent = n_node - 1
    ix[ix == absent] = 0
    row, col = [], []
    for h in hubs:
        a, b = int(ip[h]), int(ip[h + 1])
        ix[b - 1] = n_node - 2
        ix[a:b - 1][ix[a:b - 1] == n_node - 2] = 1  # the last entry's id occurs only there
        t = [ix[a], ix[b - 1], absent, ix[a + 1], ix[b - 2], ix[(a + b) // 2]]
        row += t
        col += [h] * len(t)
    row, col = np.array(row, np.uint32), np.array(col, np.uint32)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    want = run_and_check(ops, g, ip, ix, [(row, col, row.size, row.size)])[0]
    for k, h in enumerate(hubs):
        assert want[6 * k] == ip[h] and want[6 * k + 1] == ip[h + 1] - 1 and want[6 * k + 2] == EMPTY


@pytest.mark.parametrize("with_map", [False, True], ids=["global_ids", "id_map"])
def test_empty_key_and_out_of_range_ids(ops, ladder, with_map):
    """EMPTY and ids >= num_node in row and in col (through the map: also local ids beyond the map, and map entries that
    are no node) give EMPTY, and the valid edges between them their positions."""
    ip, ix, g = ladder
    row, col = layer_of(ip, ix, [(4, 70), (8, 70), (3, 70)], seed=3)
    id_map = None
    bad = [EMPTY, N, N + 5, 0x80000000]
    if with_map:
        perm = np.random.RandomState(4).permutation(N).astype(np.uint32)
        inv = np.empty(N, np.uint32)
        inv[perm] = np.arange(N, dtype=np.uint32)
        id_map = np.concatenate([perm, np.array([EMPTY, N, 0x80000000], np.uint32)])  # local N .. N + 2: no nodes
        row, col = inv[row], inv[col]
        bad = [EMPTY, N, N + 1, N + 2, N + 3, 0x80000000]  # N + 3 and up: beyond the map
    for k, b in enumerate(bad):
        row[5 + 7 * k] = b
        col[9 + 7 * k] = b
        col[80 + k] = b  # inside the long list's run: splits it
    want = run_and_check(ops, g, ip, ix, [(row, col, row.size, row.size)], id_map=id_map)[0]
    assert (want[[5 + 7 * k for k in range(len(bad))]] == EMPTY).all() and (want != EMPTY).sum() > 100


def test_three_layers_a_count_below_the_bound_and_an_empty_layer(ops, ladder):
    ip, ix, g = ladder
    r0, c0 = layer_of(ip, ix, [(9, 100), (2, 30), (7, 500), (21, 9)] * 3, seed=6)
    r2, c2 = layer_of(ip, ix, [(1, 1)], seed=7)
    cap0 = r0.size + 1000
    pr, pc = np.resize(r0, cap0), np.resize(c0, cap0)  # behind n: valid edges, which must not be touched
    layers = [(pr, pc, r0.size - 5, cap0), (r0[:40].copy(), c0[:40].copy(), 0, 40), (r2, c2, 1, 1)]
    run_and_check(ops, g, ip, ix, layers)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_arrays_that_are_not_16_byte_aligned(ops, ladder, shift):
    ip, ix, g = ladder
    row, col = layer_of(ip, ix, [(8, 130), (4, 64), (22, 5), (6, 65)], seed=shift)
    run_and_check(ops, g, ip, ix, [(row, col, row.size - 1, row.size)], shift=shift)


@pytest.mark.parametrize("cap", [1, 3])
def test_later_rounds_of_both_kernels(ops, ladder, cap):
    """13 rounds of the main kernel's grid and an odd remainder; three runs in eight are a long list's, so the long-list
    kernel has far more than 4 rounds of PARTS-workgroup units at cap 3."""
    from xgnn_amd._lib import lib
    ip, ix, g = ladder
    n = 13 * cap * UNIT + 77
    runs = []
    total = 0
    k = 0
    while total < n:
        s = [7, 2, 25, 5, 9, 30, 3, 8][k % 8]  # 7, 9, 8: long lists
        m = [5, 64, 3, 70, 9, 1, 65, 17][k % 8]
        runs.append((s, m))
        total += m
        k += 1
    row, col = layer_of(ip, ix, runs, seed=cap)
    row, col = row[:n].copy(), col[:n].copy()
    long_chunks = sum(1 for c in range(0, n, CHUNK) if np.isin(col[c:c + CHUNK], [7, 8, 9]).any())
    assert long_chunks * PARTS >= 4 * cap + 1
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        run_and_check(ops, g, ip, ix, [(row, col, n, n), (row[:300].copy(), col[:300].copy(), 299, 300)])
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


def test_positions_at_and_beyond_2_31(ops):
    """graphgen.high_offset_csr: the hub's list straddles position 2^31, the nodes behind it lie above."""
    hg = graphgen.high_offset_csr(1 << 31, seed=31)
    try:
        g = ops.DeviceGraph(dev(hg.indptr), hg.indices)
        ip = hg.indptr
        rng = np.random.RandomState(2)
        row, col = [], []
        h0, h1 = int(ip[hg.hub]), int(ip[hg.hub + 1])
        for p in [h0, h1 - 1, hg.boundary - 1, hg.boundary, hg.boundary + 1] + list(rng.randint(h0, h1, 40)):
            row.append(hg.ix[p])
            col.append(hg.hub)
        for s in list(hg.above[:40]) + list(hg.below[:40]):
            a, b = int(ip[s]), int(ip[s + 1])
            for p in range(a, min(b, a + 3)):
                row.append(hg.ix[p])
                col.append(s)
        row, col = np.array(row, np.uint32), np.array(col, np.uint32)
        want = run_and_check(ops, g, ip, hg.ix, [(row, col, row.size, row.size)], num_edge=hg.num_edge)[0]
        assert (want != EMPTY).all() and (want >= 1 << 31).sum() > 40 and (want < 1 << 31).sum() > 40
    finally:
        del hg
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_argument_errors_launch_nothing(ops, ladder):
    from xgnn_amd._lib import COUNT_EDGES, Graph, lib
    l = lib()
    ip, ix, g = ladder
    row, col = layer_of(ip, ix, [(8, 100), (4, 50)])
    n = row.size
    t_row, t_col = dev(row), dev(col)
    t_eid = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    counts = torch.zeros(11, dtype=torch.int64, device="cuda")
    counts[COUNT_EDGES(0)] = n
    me = (C.c_size_t * 1)(n)
    need = l.ggms_edge_positions_workspace_bytes(me, 1)
    assert need > 0 and l.ggms_edge_positions_workspace_bytes(me, 0) == 0 and l.ggms_edge_positions_workspace_bytes(me, 17) == 0
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    one = lambda t: (C.c_void_p * 1)(t.data_ptr() if t is not None else None)  # noqa: E731
    sharded = Graph.from_buffer_copy(g.c)
    sharded.num_part = 2
    no_indptr = Graph.from_buffer_copy(g.c)
    no_indptr.indptr = None
    base = dict(graph=C.byref(g.c), ne=ix.size, id_map=None, nmap=0, row=one(t_row), col=one(t_col), eid=one(t_eid), me=me,
                L=1, counts=ptr(counts), ws=ptr(ws), wsb=need, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    call = lambda **kw: l.ggms_edge_positions(*[kw.get(k, v) for k, v in base.items()])  # noqa: E731
    for kw, word in ((dict(graph=C.byref(sharded)), b"sharded"), (dict(ne=0xFFFFFFFF), b"32-bit"), (dict(ne=1 << 33), b"32-bit"),
                     (dict(L=0), b"num_layer"), (dict(L=17), b"num_layer"), (dict(row=None), b"invalid argument"),
                     (dict(col=None), b"invalid argument"), (dict(eid=None), b"invalid argument"),
                     (dict(me=None), b"invalid argument"), (dict(counts=None), b"invalid argument"),
                     (dict(graph=C.byref(no_indptr)), b"invalid argument"), (dict(eid=one(None)), b"null"),
                     (dict(ws=None), b"workspace"), (dict(wsb=need - 1), b"workspace")):
        assert call(**kw) == INVALID, kw
        assert word in l.ggms_last_error(), (kw, l.ggms_last_error())
    torch.cuda.synchronize()
    assert (host_u32(t_eid) == POISON).all() and ops.device_status() == 0
    assert call() == 0  # and the same arguments, all valid, do run
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(t_eid), ref.edge_positions(ip, ix, [row], [col])[0])
