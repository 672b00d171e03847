"""The ordered dedup table at its edges: the named patterns of dedup_cases.py (one key n times, chunks of owners only /
of none, duplicates across segment / round / tile / chunk boundaries) through every form of the owner scan and both
layouts, misaligned input (the scalar load paths), a hashed table at 100 % load, batches on graphs where the dedup and
not the RNG decides the outcome, and the three counters that roll over in a real run: the table version, the 30-bit
scan epoch, the 16-bit epoch of the chunk descriptors.  Everything is compared exactly with dedup_cases.reference (leaf
API) or oracle.do_sample (batches)."""
import numpy as np
import pytest

import dedup_cases as D
import oracle
import test_gpu_parity as P
from graphgen import powerlaw_csr
from dedup_cases import CASES, DIRECT_CASES, OWNER_SCAN_CHUNKS, OWNER_SCAN_TILES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NUM_KNOBS = 4  # GGMS_DEBUG_NUM_KNOBS
dev, host_u32 = P.dev, P.host_u32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as o
    return o


@pytest.fixture()
def knob():
    """test_gpu_variants.py's: set a GGMS_DEBUG_* knob for one test; every knob is back at its default afterwards."""
    from xgnn_amd import lib
    used = []

    def set_knob(which, value):
        used.append(which)
        lib().ggms_debug_set_knob(which, value)
    try:
        yield set_knob
    finally:
        for w in range(NUM_KNOBS):
            lib().ggms_debug_set_knob(w, -1)
    assert all(0 <= w < NUM_KNOBS for w in used)


@pytest.fixture(autouse=True)
def clean_status(ops):
    """every test starts from and ends with a clean device status word (the TABLE_FULL test clears what it set)"""
    assert ops.device_status(clear=True) == 0
    yield
    assert ops.device_status() == 0


# direct layout: default / the re-read form / the tile-chained kernel; hashed layout
FORMS = ["direct", "reread", "tiles", "hashed"]


def _reread_chunks(case):
    """OWNER_SCAN_CHUNKS = 24 (test_gpu_variants.py's value) re-reads a chunk only when it is longer than the two tiles a
    workgroup keeps in registers, i.e. beyond 48 tiles; the shorter patterns get as many chunks as still leaves three
    tiles in each (inputs of one or two tiles have no re-read form: they stay in registers)."""
    tiles = (max(f.size for f in case.fills) + D.TILE - 1) // D.TILE
    return 24 if tiles > 48 else max(1, tiles // 3)


def _set_form(knob, form, case):
    if form == "reread":
        knob(OWNER_SCAN_CHUNKS, _reread_chunks(case))
    elif form == "tiles":
        knob(OWNER_SCAN_TILES, 1)
    elif form == "direct" and case.chunks is not None:
        knob(OWNER_SCAN_CHUNKS, case.chunks)  # the grid the pattern's chunk boundaries are built for


def _table(ops, case, form):
    return ops.OrderedHashTable(case.capacity, num_node=None if form == "hashed" else case.num_node)


def _check_fill(ht, t_items, want, what):
    """one fill + everything the leaf API shows of it, against the reference"""
    ht.fill_with_duplicates(t_items)
    local, _ = ht.map_edges(t_items, None)
    self_map, _ = ht.map_edges(ht.unique().contiguous(), None)
    D.compare_fill(want, ht.num_items, host_u32(ht.unique()), host_u32(local), host_u32(self_map), what)


# ------------------------------------------------------------------ leaf API: every pattern x every form
# keys with bit 31 set have no word in the direct layout: `colliding` is the hashed layout's pattern
PATTERN_RUNS = [(n, f) for n in CASES for f in FORMS if f == "hashed" or CASES[n].num_node is not None]


@pytest.mark.parametrize("name,form", PATTERN_RUNS, ids=[f"{n}-{f}" for n, f in PATTERN_RUNS])
def test_pattern(ops, knob, name, form):
    case = CASES[name]
    _set_form(knob, form, case)
    ht = _table(ops, case, form)
    ht.reset()
    for i, (f, want) in enumerate(zip(case.fills, D.expected(name))):
        _check_fill(ht, dev(f), want, f"{name} / {form} / fill {i}")


@pytest.mark.parametrize("name", ["all_distinct_full_chunks-2", "boundary_pairs-chunks4", "mirrored", "all_same-100000"])
def test_pattern_with_self_served_look_backs(ops, knob, name):
    """Patience 0 (test_gpu_selfserve_scan.py): a chunk that finds an earlier chunk's word missing counts that chunk
    itself and publishes the word -- 63 488, 0 and everything between, written by owner and helpers at once."""
    from test_gpu_selfserve_scan import session_patience
    from xgnn_amd import lib
    lib().ggms_debug_set_scan_patience(0)
    try:
        test_pattern(ops, knob, name, "direct")
    finally:
        lib().ggms_debug_set_scan_patience(session_patience())


@pytest.mark.parametrize("k", [1, 2, 3])
def test_one_item_more_than_full_chunks_takes_the_tile_chain_with_the_same_result(ops, knob, k):
    """k * 63488 + 1 items under OWNER_SCAN_CHUNKS = k do not fit k chunks (chunk_fits): the tile-chained kernel runs and
    must give what the chunked kernel gives for the same array (and both what the reference says)."""
    case = CASES[f"all_distinct_full_chunks-{k}-plus1"]
    want = D.expected(case.name)
    got = {}
    for form in ("direct", "reread"):  # "direct" = k chunks: does not fit; "reread" = 24 chunks of 2 .. 4 tiles: fits
        _set_form(knob, form, case)
        ht = _table(ops, case, form)
        ht.reset()
        for i, (f, w) in enumerate(zip(case.fills, want)):
            _check_fill(ht, dev(f), w, f"{case.name} / {form} / fill {i}")
        got[form] = host_u32(ht.unique()).copy()
        knob(OWNER_SCAN_CHUNKS, -1)
    np.testing.assert_array_equal(got["direct"], got["reread"])


# ------------------------------------------------------------------ misaligned input: the scalar load paths
MISALIGNED = ["all_same-2048", "all_same-2049", "boundary_pairs", "boundary_pairs-chunks3", "boundary_pairs-chunks4", "mirrored",
              "strided-129", "strided-2048", "runs-513", "descending", "all_distinct_full_chunks-1", "all_distinct_register_chunks"]
assert set(MISALIGNED) <= set(DIRECT_CASES) and {CASES[n].fills[0].size % 2 for n in MISALIGNED} == {0, 1}  # odd and even n


@pytest.mark.parametrize("form", FORMS[:3])
@pytest.mark.parametrize("name", MISALIGNED)
def test_misaligned_input(ops, knob, name, form):
    """The fills as t[1:], a view 4 bytes off a 16-byte boundary: `items` fails the owner scans' vec_ok test (8-byte
    loads in the chunked kernel, 16-byte loads in the tile-chained one) and every stream is read by the scalar path.
    Odd and even n."""
    case = CASES[name]
    _set_form(knob, form, case)
    ht = _table(ops, case, form)
    ht.reset()
    for i, (f, want) in enumerate(zip(case.fills, D.expected(name))):
        t = dev(np.concatenate([np.zeros(1, np.uint32), f]))[1:]
        assert t.data_ptr() % 8 == 4 and t.is_contiguous() and t.numel() == f.size
        _check_fill(ht, t, want, f"{name} / {form} / misaligned fill {i}")


# ------------------------------------------------------------------ hashed layout at 100 % load
def test_hashed_table_filled_to_the_last_bucket(ops):
    """64 keys that all probe from bucket 0 of a 64-bucket table: the last one entered needs mask + 1 = 64 steps of the
    triangular probe sequence, in find_or_claim and again in find.  Exact results, status 0.  A 65th key then finds no
    bucket: GGMS_STATUS_TABLE_FULL, and nothing that was there changes."""
    case = CASES["colliding-64"]
    keys = case.marks["keys"]
    ht = ops.OrderedHashTable(80)  # TableSize(80) = 256 buckets, n2o of 80 entries
    assert ht.c.o2n_size >= 64 and ht.n2o.numel() >= 65
    ht.c.o2n_size = 64  # the struct is the caller's plain data: 64 of the initialised buckets
    ht.reset()
    want = D.expected(case.name)
    for i, (f, w) in enumerate(zip(case.fills, want)):
        _check_fill(ht, dev(f), w, f"100 % load / fill {i}")
        assert ht.num_items == 64 and ops.device_status() == 0
    ids, _ = ht.map_edges(dev(keys), None)  # every key is found, the one behind 64 probes included
    np.testing.assert_array_equal(np.sort(host_u32(ids)), np.arange(64, dtype=np.uint32))
    before = host_u32(ht.unique()).copy()
    extra = np.array([keys[0], 64 * 64, keys[63]], np.uint32)  # 4096 probes from bucket 0 too
    assert extra[1] not in keys and extra[1] & 63 == 0
    ht.fill_with_duplicates(dev(extra))
    assert ops.device_status() & 2  # GGMS_STATUS_TABLE_FULL
    assert ht.num_items == 64
    np.testing.assert_array_equal(host_u32(ht.unique()), before)
    again, _ = ht.map_edges(dev(keys), None)
    np.testing.assert_array_equal(host_u32(again), host_u32(ids))
    assert ops.device_status(clear=True) & 2
    assert ops.device_status() == 0


# ------------------------------------------------------------------ batch mode: graphs where the dedup decides
def _csr(lists):
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum([len(x) for x in lists])
    ix = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if ip[-1] else np.zeros(0, np.uint32)
    return ip, np.ascontiguousarray(ix, np.uint32)


def funnel_graph(n=6000, f=5):
    """every node's list is the same f nodes: a layer of m inputs is m * f copies of f keys"""
    hub = [(n // 2 + 37 * j) % n for j in range(f)]
    return _csr([hub] * n)


def tree_graph(n=20_000, f=3):
    """f-ary heap order, children of v = f v + 1 .. f v + f: no neighbour is shared, every new item owns its key"""
    return _csr([[c for c in range(f * v + 1, f * v + f + 1) if c < n] for v in range(n)])


def ring_graph(n=12_000):
    """v -> v + 1 only: seeds that are not adjacent never share a neighbour inside a layer; a later layer samples the
    earlier layers' nodes again, so every duplicate is one across layers (cand >= 2)"""
    return _csr([[(v + 1) % n] for v in range(n)])


GRAPHS = {}


def _graph(ops, which):
    if which not in GRAPHS:
        ip, ix = {"funnel": funnel_graph, "tree": tree_graph, "ring": ring_graph}[which]()
        GRAPHS[which] = (ip, ix, ops.DeviceGraph(dev(ip), dev(ix)), dev(ix))
    return GRAPHS[which]


def _seeds(which, nseed, rep):
    rng = np.random.RandomState(1000 * rep + nseed)
    if which == "tree":  # one level of the heap (364 .. 1092): no seed is another seed's descendant within two layers
        return (364 + rng.permutation(729)[:nseed]).astype(np.uint32)
    if which == "ring":  # multiples of 4: never adjacent, and their 3-hop chains stop short of the next seed
        return (4 * rng.permutation(3000)[:nseed]).astype(np.uint32)
    return rng.permutation(6000)[:nseed].astype(np.uint32)


def _batch_equal(got, want, L, what):
    np.testing.assert_array_equal(host_u32(got["input_nodes"]), want["input_nodes"], err_msg=f"{what}: input nodes")
    for i in range(L):
        gl, wl = got["layers"][i], want["layers"][i]
        assert (gl["num_src"], gl["num_dst"]) == (wl["num_src"], wl["num_dst"]), (what, i)
        np.testing.assert_array_equal(host_u32(gl["row"]), wl["row"], err_msg=f"{what}: row layer {i}")
        np.testing.assert_array_equal(host_u32(gl["col"]), wl["col"], err_msg=f"{what}: col layer {i}")


def _sampler(ops, which, stype, fanouts, nseed, direct, seed=31):
    ip, ix, g, _ = _graph(ops, which)
    code, ocode = {"khop3": (ops.KHOP3, oracle.KHOP3), "khop0": (ops.KHOP0, oracle.KHOP0)}[stype]
    bs = ops.BatchSampler(g, fanouts, nseed, sample_type=code, seed=seed, direct_table=direct)
    st = oracle.random_states(bs.states.shape[0], seed) if stype != "khop0" else None
    return bs, lambda seeds: oracle.do_sample(ocode, ip, ix, seeds, fanouts, st)


BATCHES = [("funnel", [5, 5], 1000), ("funnel", [5, 5], 301), ("tree", [3, 3], 301), ("tree", [3], 700), ("ring", [3, 3, 3], 1000),
           ("ring", [3, 3, 3], 301)]


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["khop3", "khop0"])
@pytest.mark.parametrize("which,fanouts,nseed", BATCHES, ids=[f"{w}-{'-'.join(map(str, f))}-{n}" for w, f, n in BATCHES])
def test_batch_on_dedup_graphs(ops, which, fanouts, nseed, stype, direct):
    """Every degree is at most the fanout, so a layer is the whole neighbourhood and only the dedup shapes the batch:
    funnel = a layer of n * F items is F keys; tree = every new item owns; ring = duplicates only across layers.
    301 seeds with fanout 3 / 5: the layers' index bases (301, 301 + 903, ...) are odd."""
    ip, ix, _, t_ix = _graph(ops, which)
    assert ip.size - 1 <= 20_000 and nseed <= 1000 and int(np.diff(ip.astype(np.int64)).max()) <= min(fanouts)
    bs, want_of = _sampler(ops, which, stype, fanouts, nseed, direct)
    for rep in range(2):
        seeds = _seeds(which, nseed, rep)
        assert np.unique(seeds).size == nseed
        bs.sample(dev(seeds))
        want = want_of(seeds)
        _batch_equal(bs.result(), want, len(fanouts), f"{which} {stype} rep {rep}")
        if which == "funnel":  # the property the graph is named for: F keys behind the seeds
            assert want["input_nodes"].size <= nseed + fanouts[0]
        if which == "tree":    # nothing is shared: every sampled edge of the first layer is a new node
            assert want["layers"][-1]["num_src"] == nseed + want["layers"][-1]["row"].size
        if which == "ring":    # one new node per chain and layer
            assert want["input_nodes"].size == nseed * (1 + len(fanouts))
    np.testing.assert_array_equal(host_u32(t_ix), ix)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["khop3", "khop0"])
@pytest.mark.parametrize("which", ["funnel", "tree"])
def test_batch_of_one_seed_a_thousand_times(ops, which, stype, direct):
    """1000 copies of one node as the seeds: the seeds' fill is all_same, the first layer 1000 copies of one list."""
    bs, want_of = _sampler(ops, which, stype, [5, 5] if which == "funnel" else [3, 3], 1000, direct)
    for node in (500, 17):
        seeds = np.full(1000, node, np.uint32)
        bs.sample(dev(seeds))
        want = want_of(seeds)
        _batch_equal(bs.result(), want, 2, f"{which} {stype} seed {node} x 1000")
        assert want["layers"][-1]["num_dst"] == 1000 and want["input_nodes"][0] == node


# ------------------------------------------------------------------ version rollover
V_LAST = 0x7FFFFFF0  # a table at this version is re-initialised by its next reset (hashtable.hip, sample_batch.hip)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_version_rollover_leaf(ops, direct):
    """ggms_hashtable_reset's copy of the re-initialisation: versions 0x7fffffef, 0x7ffffff0, then init -> 1, 2.  Round 0
    ran at version 1 too (before the jump): without the re-init its words would be version-1 words of round 3's table.
    The rounds' key sets overlap, in another order each time."""
    N, n = 6000, 5000
    ht = ops.OrderedHashTable(4 * n + 16, num_node=N if direct else None)
    rng = np.random.RandomState(4)
    fills = [rng.randint(0, N // 2, n).astype(np.uint32)]                      # round 0: keys of the lower half
    fills += [rng.randint(r * 500, r * 500 + N // 2, n).astype(np.uint32) for r in range(1, 5)]  # shifted windows: overlapping
    fills[3] = np.concatenate([fills[0][::-1][:n // 2], fills[3][:n // 2]])   # round 3 (version 1 again) re-enters round 0's keys
    ht.reset()
    assert ht.c.version == 1
    _check_fill(ht, dev(fills[0]), D.reference([fills[0]])[0], "round 0")
    ht.c.version = 0x7FFFFFEE
    versions = []
    for r in range(1, 5):
        ht.reset()
        versions.append(ht.c.version)
        want = D.reference([fills[r]])[0]  # a reset table knows nothing of the earlier rounds
        _check_fill(ht, dev(fills[r]), want, f"round {r} at version {ht.c.version:#x}")
        stale = set(np.concatenate(fills[:r]).tolist()) - set(fills[r].tolist())
        assert stale and not (stale & set(host_u32(ht.unique()).tolist())), r
    assert versions == [0x7FFFFFEF, V_LAST, 1, 2]


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["khop3", "khop0"])
def test_version_rollover_batch(ops, stype, direct):
    """ggms_sample_batch's copy: four batches across the re-initialisation, each the oracle's."""
    ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
    g = ops.DeviceGraph(dev(ip), dev(ix))
    fanouts, nseed = [5, 10], 300
    code, ocode = {"khop3": (ops.KHOP3, oracle.KHOP3), "khop0": (ops.KHOP0, oracle.KHOP0)}[stype]
    bs = ops.BatchSampler(g, fanouts, nseed, sample_type=code, seed=13, direct_table=direct)
    st = oracle.random_states(bs.states.shape[0], 13) if stype != "khop0" else None
    rng = np.random.RandomState(6)
    versions = []
    for b in range(5):
        if b == 1:
            torch.cuda.synchronize()
            bs.hts[0].c.version = 0x7FFFFFEE
        seeds = rng.permutation(2000)[:nseed].astype(np.uint32)  # a small universe: the batches' key sets overlap
        bs.sample(dev(seeds))
        versions.append(bs.hts[0].c.version)
        _batch_equal(bs.result(), oracle.do_sample(ocode, ip, ix, seeds, fanouts, st), 2, f"batch {b} at version {versions[-1]:#x}")
    assert versions == [1, 0x7FFFFFEF, V_LAST, 1, 2]


# ------------------------------------------------------------------ scan epochs
class scan_epoch:
    """with scan_epoch(counter): the process-wide launch counter behind the scans' epochs is `counter` inside and what
    it was before afterwards -- later scans never repeat an epoch this test left in device memory."""

    def __init__(self, counter):
        self.counter = counter

    def __enter__(self):
        from xgnn_amd import lib
        self.saved = lib().ggms_debug_set_scan_epoch(self.counter)
        return self

    def __exit__(self, *exc):
        from xgnn_amd import lib
        torch.cuda.synchronize()
        self.left = lib().ggms_debug_set_scan_epoch(self.saved)
        return False


def test_set_scan_epoch_returns_the_previous_counter(ops):
    from xgnn_amd import lib
    saved = lib().ggms_debug_set_scan_epoch(0x12345)
    try:
        assert lib().ggms_debug_set_scan_epoch(0x23456) == 0x12345
        ht = ops.OrderedHashTable(64, num_node=64)
        ht.reset()
        ht.fill_with_duplicates(dev(np.arange(10, dtype=np.uint32)))  # one owner scan = one epoch
        assert lib().ggms_debug_set_scan_epoch(7) == 0x23457
    finally:
        assert lib().ggms_debug_set_scan_epoch(saved) == 7


def _eight_fills(ops, direct, what, n=5000):
    N = 4000
    rng = np.random.RandomState(8)
    fills = [rng.randint(0, N, n).astype(np.uint32) for _ in range(8)]
    want = D.reference(fills)
    ht = ops.OrderedHashTable(8 * n, num_node=N if direct else None)
    ht.reset()
    for i in range(8):
        _check_fill(ht, dev(fills[i]), want[i], f"{what} fill {i}")
    assert ops.device_status() == 0


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_scan_epoch_30_bit_wrap(ops, direct):
    """Eight fills (three tiles / chunks each) from counter 0x3ffffffc: epochs 0x3ffffffd .. 0x3fffffff, the skipped 0
    (a cleared descriptor's epoch), 1 ..  The leaf API clears its scan area on every call, so the outcome does not
    depend on what ran before."""
    with scan_epoch(0x3FFFFFFC) as e:
        _eight_fills(ops, direct, f"30-bit wrap ({'direct' if direct else 'hashed'})")
    assert e.left == 0x3FFFFFFC + 9  # eight epochs and the skipped one: the wrap was crossed


def _band(k):
    """a counter base near 0x20000000 with (B + 3) % 65535 == 0, one band per case (16 x 65535 apart): no two cases
    share an epoch"""
    b = 0x20000000 + 16 * 65535 * k
    b += (-(b + 3)) % 65535
    assert (b + 3) % 65535 == 0 and 0x20000000 <= b < 0x3F000000
    return b


@pytest.mark.parametrize("what,k", [("leaf", 0), ("leaf-reread", 1), ("batch", 2)])
def test_chunk_epoch_16_bit_wrap(ops, knob, what, k):
    """The chunk descriptors carry epoch % 65535 + 1 in 16 bits: 65534, 65535, 1, 2 ... across B + 3.  A real run crosses
    this every few thousand batches."""
    B = _band(k)
    assert [(B + i) % 65535 + 1 for i in (1, 2, 3, 4)] == [65534, 65535, 1, 2]
    with scan_epoch(B) as e:
        if what == "batch":
            ip, ix = powerlaw_csr(20_000, mean_deg=30, seed=2)
            g = ops.DeviceGraph(dev(ip), dev(ix))
            fanouts, nseed = [5, 10, 15], 300
            bs = ops.BatchSampler(g, fanouts, nseed, sample_type=ops.KHOP3, seed=3, direct_table=True)
            st = oracle.random_states(bs.states.shape[0], 3)
            rng = np.random.RandomState(k)
            for b in range(6):
                seeds = rng.permutation(20_000)[:nseed].astype(np.uint32)
                bs.sample(dev(seeds))
                _batch_equal(bs.result(), oracle.do_sample(oracle.KHOP3, ip, ix, seeds, fanouts, st), 3, f"batch {b}")
        else:
            if what == "leaf-reread":
                knob(OWNER_SCAN_CHUNKS, 2)  # 13 000 items = 7 tiles in two chunks of 4 and 3: the re-read form
            _eight_fills(ops, True, what, n=13_000 if what == "leaf-reread" else 5000)
    assert e.left >= B + 6  # the wrap at B + 3 lies inside what ran
