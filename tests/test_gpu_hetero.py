"""ggms_hetero_nodes / ggms_hetero_edges on the GPU against their numpy statement (tests/hetero_ref.py), bit for bit, on
hand-built batches -- no sampler.  Guard words lie around every output and poison behind what a call may write; no counts
word is written; the device status stays 0.

xgnn_amd/csrc/hetero.hip: a workgroup takes a TILE of 2048 items per round, each of its four waves eight CHUNKs of 64; a
job (the node list, a layer) has at least one tile; histograms of at most 1024 words are scanned by one workgroup, larger
ones by the tiled scan."""
import numpy as np
import pytest

import hetero_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHUNK, TILE = 64, 2048
EMPTY = ref.EMPTY
GUARD = 0x5A5A5A5A
POISON = 0x0BADBEEF
GUARD8, POISON8 = 0x5A, 0xEE
GRID_CAP = 3  # GGMS_DEBUG_GRID_CAP
PAD = 64
NUM_NODE = 5000


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


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


class Guarded:
    """`cap` poisoned elements behind `shift` guard elements and in front of PAD more."""

    def __init__(self, cap, shift=0, dtype=torch.int32):
        guard, poison = (GUARD, POISON) if dtype == torch.int32 else (GUARD8, POISON8)
        self.cap, self.shift, self.guard, self.poison = cap, shift, guard, poison
        self.buf = torch.full((shift + cap + PAD,), guard, dtype=dtype, device="cuda")
        self.buf[shift:shift + cap] = poison
        self.t = self.buf[shift:shift + cap]

    def check(self, want, what):
        """the first len(want) elements are `want`, the rest of the cap is poison, the guards are whole"""
        h = host(self.buf)
        g, p = h.dtype.type(self.guard), h.dtype.type(self.poison)
        s, n = self.shift, len(want)
        assert n <= self.cap, what
        np.testing.assert_array_equal(h[s:s + n], want, err_msg=what)
        assert (h[s + n:s + self.cap] == p).all(), f"{what}: written behind its end"
        assert (h[:s] == g).all() and (h[s + self.cap:] == g).all(), f"{what}: a guard word is gone"


# ---- the nodes ---------------------------------------------------------------------------------------------------------
def node_types(T, seed=0, absent=None):
    rng = np.random.RandomState(100 + seed)
    nt = rng.randint(0, T, NUM_NODE).astype(np.uint8)
    if absent is not None:
        nt[nt == absent] = (absent + 1) % T
    return nt


def nodes_with_types(node_type, want_types, seed=0):
    """ids whose types are exactly want_types (0xFF: an id that is no node)"""
    rng = np.random.RandomState(200 + seed)
    out = np.empty(len(want_types), np.uint32)
    bad = [EMPTY, NUM_NODE, NUM_NODE + 17, 0x80000000]
    for t in np.unique(want_types):
        at = np.flatnonzero(want_types == t)
        pool = np.array(bad, np.uint32) if t == ref.NO_TYPE else np.flatnonzero(node_type == t).astype(np.uint32)
        assert pool.size
        out[at] = pool[rng.randint(0, pool.size, at.size)]
    return out


def run_nodes(ops, node_type, T, nodes, n, cuts, cap=None, shift=0, workspace=None, check=True):
    """nodes: cap entries of which the first n count (the device count says n).  -> a closure that checks the outputs."""
    cap = nodes.size if cap is None else cap
    assert nodes.size == cap and n <= cap
    B = len(cuts)
    counts = np.arange(9000, 9000 + 40, dtype=np.int64)
    words = [2 * k + 3 for k in range(B)]  # scattered words of a larger counts array
    for w, c in zip(words, cuts):
        counts[w] = c
    counts[1] = n
    t_counts = torch.from_numpy(counts.copy()).cuda()
    t_nodes = dev(nodes)
    out = dict(ntype=Guarded(cap, shift, torch.uint8), local=Guarded(cap, shift), slot=Guarded(cap, shift),
               typed_nodes=Guarded(cap, shift), base=Guarded(T + 1), cut_counts=Guarded(B * T))
    got = ops.hetero_nodes(dev(node_type), T, t_nodes, num_nodes_dev=t_counts[1:2], cut_base=t_counts, cut_words=words,
                           max_nodes=cap, out={k: v.t for k, v in out.items()}, workspace=workspace)
    assert got["local"].data_ptr() == out["local"].t.data_ptr()
    want = ref.hetero_nodes(node_type, T, nodes[:n], cuts)

    def verify():
        np.testing.assert_array_equal(t_counts.cpu().numpy(), counts)
        np.testing.assert_array_equal(host(t_nodes), nodes)
        for name in ("ntype", "local", "slot", "typed_nodes", "base"):
            out[name].check(want[name], name)
        out["cut_counts"].check(want["cut_counts"].reshape(-1), "cut_counts")
        assert ops.device_status() == 0
        return want

    return verify() if check else verify


SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5]


@pytest.mark.parametrize("T", [1, 2, 5, 32])
@pytest.mark.parametrize("n", SIZES)
def test_nodes_sizes_types_invalid_ids_and_cuts(ops, n, T):
    """Random types with ids that are no node among them, a device count below max_nodes, cuts at 0, 1, n, above n and on
    tile boundaries."""
    nt = node_types(T, seed=T)
    rng = np.random.RandomState(n + T)
    cap = n + 300
    nodes = rng.randint(0, NUM_NODE, cap).astype(np.uint32)  # behind n: valid ids, which must not be looked at
    for k, b in enumerate([EMPTY, NUM_NODE, NUM_NODE + 1, 0x80000000]):
        if n > 5:
            nodes[rng.randint(0, n)] = b
        if n > 70:
            nodes[64 - k] = b
    cuts = [0, 1, n, n + 7, n // 2, 2048, 4096, 6144, 2047, 1 << 40]
    want = run_nodes(ops, nt, T, nodes, n, cuts, cap=cap)
    if n > 70:
        assert (want["ntype"][61:65] == ref.NO_TYPE).all() and (want["slot"][61:65] == EMPTY).all()


def pattern(name, T, n):
    i = np.arange(n)
    if name == "one_type":
        return np.full(n, T - 1, np.uint8)
    if name == "alternating":
        return (i % T).astype(np.uint8)
    if name == "last_tile_only":  # type 1 shows up in the last tile only
        t = np.where(i % 3 == 0, 0, 2).astype(np.uint8)
        t[-3:] = 1
        return t
    if name == "runs_end_at_63_64":
        return ((i // 64) % T).astype(np.uint8)
    if name == "runs_end_at_2047_2048":
        return ((i // 2048) % T).astype(np.uint8)
    if name == "all_invalid":
        return np.full(n, ref.NO_TYPE, np.uint8)
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["one_type", "alternating", "absent_type", "last_tile_only", "runs_end_at_63_64",
                                  "runs_end_at_2047_2048", "all_invalid"])
def test_nodes_type_patterns(ops, name):
    T, n = 5, 2 * 2048 + 70
    if name == "absent_type":
        nt = node_types(T, seed=1, absent=2)
        nodes = np.random.RandomState(3).randint(0, NUM_NODE, n).astype(np.uint32)
    else:
        nt = node_types(T, seed=2)
        nodes = nodes_with_types(nt, pattern(name, T, n))
    want = run_nodes(ops, nt, T, nodes, n, [64, 2048, n])
    sizes = np.diff(want["base"])
    if name == "absent_type":
        assert sizes[2] == 0 and sizes.sum() == n
    if name == "one_type":
        assert sizes.tolist() == [0, 0, 0, 0, n]
        np.testing.assert_array_equal(want["typed_nodes"], nodes)
    if name == "last_tile_only":
        assert sizes[1] == 3 and want["cut_counts"][1][1] == 0
    if name == "all_invalid":
        assert want["base"][T] == 0


@pytest.mark.parametrize("cap", [1, 3])
def test_nodes_later_rounds_of_the_grid(ops, cap):
    """8 tiles on 1 / 3 workgroups; T = 32 makes the histogram (8 x 33 words) one small scan, the second shape (40 tiles,
    1320 words) takes the tiled scan."""
    from xgnn_amd._lib import lib
    nt = node_types(32, seed=5)
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        for n in (7 * TILE + 5, 39 * TILE + 1000):
            nodes = np.random.RandomState(n % 97).randint(0, NUM_NODE + 40, n).astype(np.uint32)
            run_nodes(ops, nt, 32, nodes, n, [n - 1, 5 * TILE, 17])
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_nodes_outputs_off_a_16_byte_boundary(ops, shift):
    nt = node_types(3, seed=7)
    nodes = np.random.RandomState(shift).randint(0, NUM_NODE, 2300).astype(np.uint32)
    run_nodes(ops, nt, 3, nodes, 2211, [100], shift=shift)


def test_nodes_without_cuts_or_device_count(ops):
    nt = node_types(4, seed=8)
    nodes = np.random.RandomState(1).randint(0, NUM_NODE, 700).astype(np.uint32)
    got = ops.hetero_nodes(dev(nt), 4, dev(nodes))
    want = ref.hetero_nodes(nt, 4, nodes)
    for name in ("ntype", "local", "slot", "typed_nodes", "base"):
        np.testing.assert_array_equal(host(got[name])[:want[name].size], want[name], err_msg=name)
    assert ops.device_status() == 0


# ---- the edges ---------------------------------------------------------------------------------------------------------
def typed_runs(E, R, seed, over=0):
    """types as khop_typed emits them: ascending inside a seed's run, unsorted across the array; `over`: that many entries
    with a type >= R."""
    rng = np.random.RandomState(300 + seed)
    out = np.empty(E, np.uint8)
    at = 0
    while at < E:
        m = min(E - at, int(rng.randint(1, 24)))
        out[at:at + m] = np.sort(rng.randint(0, R, m))
        at += m
    if over and E:
        out[rng.randint(0, E, over)] = rng.randint(R, 256, over)
    return out


def make_layer(E, R, seed, num_local, cap=None, etype=None, over=0):
    rng = np.random.RandomState(400 + seed)
    cap = E if cap is None else cap
    row = rng.randint(0, num_local, cap).astype(np.uint32)
    col = rng.randint(0, num_local, cap).astype(np.uint32)
    eid = rng.randint(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32)
    et = typed_runs(cap, R, seed, over) if etype is None else np.resize(etype, cap).astype(np.uint8)
    if E > 10:
        row[3], col[7], row[E - 1] = num_local, EMPTY, num_local + 5  # beyond `local`: EMPTY comes out
    return row, col, eid, et, E, cap


def run_edges(ops, layers, R, local, with_eid=True, shift=0, et_shift=0, workspace=None, check=True):
    """layers: [(row, col, eid, etype, E, cap)] -- the arrays hold cap entries, the first E count."""
    from xgnn_amd import _lib
    L = len(layers)
    counts = np.arange(7000, 7000 + _lib.COUNTS_WORDS(L), dtype=np.int64)
    for i, lay in enumerate(layers):
        counts[_lib.COUNT_EDGES(i)] = lay[4]
    t_counts = torch.from_numpy(counts.copy()).cuda()
    caps = [lay[5] for lay in layers]
    rows, cols, eids = ([dev(lay[j]) if lay[5] else torch.zeros(1, dtype=torch.int32, device="cuda") for lay in layers]
                        for j in range(3))
    ets = []
    for lay in layers:  # etype starts et_shift bytes behind an aligned allocation
        t = torch.zeros(et_shift + lay[5] + 1, dtype=torch.uint8, device="cuda")
        t[et_shift:et_shift + lay[5]] = dev(lay[3])
        ets.append(t[et_shift:et_shift + lay[5] + 1])
        assert ets[-1].data_ptr() % 16 == et_shift
    outs = [[Guarded(c, shift) for c in caps] for _ in range(3)]
    assert all(g.t.data_ptr() % 16 == 4 * shift for o in outs for g in o)
    off = Guarded(L * (R + 1))
    t_local = dev(local)
    got = ops.hetero_edges(rows, cols, ets, R, t_counts, t_local, eids=eids if with_eid else None, max_edges=caps,
                           out=([g.t for g in outs[0]], [g.t for g in outs[1]], [g.t for g in outs[2]] if with_eid else None),
                           rel_offsets=off.t, workspace=workspace)
    assert got[3].data_ptr() == off.t.data_ptr()
    want = ref.hetero_edges([lay[0][:lay[4]] for lay in layers], [lay[1][:lay[4]] for lay in layers],
                            [lay[2][:lay[4]] for lay in layers] if with_eid else None, [lay[3][:lay[4]] for lay in layers],
                            R, local)

    def verify():
        np.testing.assert_array_equal(t_counts.cpu().numpy(), counts)
        off.check(want[3].reshape(-1), "rel_offsets")
        for i in range(L):
            outs[0][i].check(want[0][i], f"out_row of layer {i}")
            outs[1][i].check(want[1][i], f"out_col of layer {i}")
            outs[2][i].check(want[2][i] if with_eid else [], f"out_eid of layer {i}")
            np.testing.assert_array_equal(host(rows[i])[:caps[i]], layers[i][0][:caps[i]])  # the inputs are read only
        assert ops.device_status() == 0
        return want

    return verify() if check else verify


@pytest.fixture(scope="module")
def local_map():
    rng = np.random.RandomState(11)
    return rng.randint(0, 1 << 20, 3000).astype(np.uint32)


EDGE_SIZES = [0, 1, 64, 65, 2048, 2049, 10007]


@pytest.mark.parametrize("R", [1, 2, 5, 32])
@pytest.mark.parametrize("E", EDGE_SIZES)
def test_edges_sizes_and_relations(ops, local_map, E, R):
    """Types sorted only inside a seed's run, a few entries with a type >= R, a count below the bound."""
    lay = make_layer(E, R, E + R, local_map.size, cap=E + 200, over=min(E, 5))
    want = run_edges(ops, [lay], R, local_map)
    assert want[3][0, R] == (lay[3][:E] < R).sum()


@pytest.mark.parametrize("name", ["one_relation", "absent_relation", "all_over", "alternating", "runs_end_at_63_64"])
def test_edges_type_patterns(ops, local_map, name):
    R, E = 5, 2 * TILE + 333
    i = np.arange(E)
    et = {"one_relation": np.full(E, 3), "absent_relation": np.where(typed_runs(E, R, 1) == 2, 4, typed_runs(E, R, 1)),
          "all_over": np.full(E, R), "alternating": i % R, "runs_end_at_63_64": (i // 64) % R}[name].astype(np.uint8)
    want = run_edges(ops, [make_layer(E, R, 2, local_map.size, etype=et)], R, local_map)
    sizes = np.diff(want[3][0].astype(np.int64))
    if name == "one_relation":
        assert sizes.tolist() == [0, 0, 0, E, 0]
    if name == "absent_relation":
        assert sizes[2] == 0 and sizes.sum() == E
    if name == "all_over":
        assert sizes.sum() == 0


def test_edges_without_ids(ops, local_map):
    run_edges(ops, [make_layer(3000, 4, 5, local_map.size, over=3)], 4, local_map, with_eid=False)


def test_edges_three_layers_one_of_them_empty(ops, local_map):
    layers = [make_layer(5000, 4, 6, local_map.size, cap=5500), make_layer(0, 4, 7, local_map.size, cap=40),
              make_layer(70, 4, 8, local_map.size)]
    want = run_edges(ops, layers, 4, local_map)
    assert want[3][1].tolist() == [0] * 5 and want[3][2][4] == 70
    run_edges(ops, [make_layer(0, 4, 9, local_map.size)], 4, local_map)  # a bound of 0: null-sized arrays, offsets of 0


@pytest.mark.parametrize("et_shift", [1, 3, 7])
def test_edges_types_from_a_misaligned_base(ops, local_map, et_shift):
    run_edges(ops, [make_layer(2500, 5, et_shift, local_map.size, over=2)], 5, local_map, et_shift=et_shift)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_edges_outputs_off_a_16_byte_boundary(ops, local_map, shift):
    run_edges(ops, [make_layer(2500, 5, shift, local_map.size), make_layer(65, 5, shift + 9, local_map.size)], 5, local_map,
              shift=shift)


@pytest.mark.parametrize("cap", [1, 3])
def test_edges_later_rounds_of_the_grid(ops, local_map, cap):
    """11 tiles in three layers on 1 / 3 workgroups, then 40 tiles x 33 rows: the tiled scan."""
    from xgnn_amd._lib import lib
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        layers = [make_layer(7 * TILE + 9, 5, 20, local_map.size, over=9), make_layer(TILE, 5, 21, local_map.size),
                  make_layer(2 * TILE + 1, 5, 22, local_map.size, cap=3 * TILE)]
        run_edges(ops, layers, 5, local_map)
        run_edges(ops, [make_layer(39 * TILE + 77, 32, 23, local_map.size, over=4)], 32, local_map)
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


def test_edges_histogram_beyond_the_single_pass_scan(ops, local_map):
    """33 rows x 7950 tiles are more than 256 scan tiles of 1024 words: the scan takes its three-launch form."""
    E, R = 7950 * TILE - 11, 32
    rng = np.random.RandomState(6)
    row = rng.randint(0, local_map.size, E).astype(np.uint32)
    et = rng.randint(0, R + 1, E).astype(np.uint8)
    want = run_edges(ops, [(row, row[::-1].copy(), row, et, E, E)], R, local_map, with_eid=False)
    assert want[3][0, R] == (et < R).sum()


# ---- both --------------------------------------------------------------------------------------------------------------
def test_two_calls_of_each_leaf_on_one_workspace(ops, local_map):
    """Back to back on one stream, nothing in between: the second call's scan reuses the first one's words."""
    from xgnn_amd._lib import lib
    import ctypes as C
    need = max(lib().ggms_hetero_nodes_workspace_bytes(41 * TILE, 32),
               lib().ggms_hetero_edges_workspace_bytes((C.c_size_t * 1)(41 * TILE), 1, 32))
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device="cuda")
    rng = np.random.RandomState(4)
    checks = []
    for n, T in ((40 * TILE + 3, 32), (40 * TILE + 3, 32), (5000, 5), (100, 5)):
        nodes = rng.randint(0, NUM_NODE, n).astype(np.uint32)
        checks.append(run_nodes(ops, node_types(T, seed=T), T, nodes, n, [n // 3], workspace=ws, check=False))
    for E, R in ((40 * TILE + 3, 32), (40 * TILE + 3, 32), (5000, 5), (100, 5)):
        checks.append(run_edges(ops, [make_layer(E, R, E % 50 + R, local_map.size)], R, local_map, workspace=ws, check=False))
    for c in checks:
        c()
