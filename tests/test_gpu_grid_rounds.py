"""Every grid-stride kernel's LATER rounds, through the library's grid cap (ggms_debug_set_knob(GGMS_DEBUG_GRID_CAP),
include/ggms.h): with at most 1 or 3 workgroups per launch a few thousand items take a kernel through what it otherwise
needs hundreds of thousands for -- the next-tile prefetch hand-over, LDS words reused behind a loop's closing barrier,
and the ticketed forms taken only when there are fewer workgroups than tiles.

  cap 1: ONE workgroup does every round (the most reuse of LDS and of carried registers);
  cap 3: an odd stride, several workgroups racing, and a partial last round.

A case is sized so that a workgroup gets at least 4 rounds at cap 3 with the last round partial: at least
13 x (items per workgroup round) + an odd remainder; the per-round unit stands next to each case.  The batch cases keep
their 1000 seeds, so the kernels that only see a batch's seeds get fewer rounds there (k_seed_enter: 2 at cap 3) and
their four rounds from a case of their own.  Not run here: k_copy_words and k_probe_index (plain element loops through
grid_for) and k_copy_prefix (a fixed grid of 256 workgroups); DESIGN.md 8g has the whole table.  Expected values are
the ones the suite already has (the oracle, the numpy twins, the families of feat_formats): the checks are the existing
tests' own, called with these sizes, so results are compared bit for bit, with RNG pools, counts and status words
wherever the leaf tests compare them.  Two cases at the end run WITHOUT the knob at the sizes where update_rows' and the
gather's own grid clamps (512 and 256 workgroups) start a second round."""
import numpy as np
import pytest

import gather_harness as GH
import oracle
import test_gpu_arch3 as A3
import test_gpu_arch4 as A4
import test_gpu_arch5 as A5
import test_gpu_device_counts as DC
import test_gpu_drop_pair_edges as DROP
import test_gpu_khop_labor as LABOR
import test_gpu_link_seeds as LINK
import test_gpu_owner_split as OWNER
import test_gpu_parity as P
import test_gpu_presample_static as CLOSURE
import test_gpu_quantize_rows as Q
import test_gpu_selfserve_scan as SCAN
import test_gpu_update_rows as UPD
import test_gpu_variants as V
import test_gpu_weighted_tables as WT
from feat_formats import BF16, E4M3, F16, F32, FAMILY, Q8ROW, assert_bits, assert_fp8_bytes, cpu_q8row, from_f32, tensor_bits
from graphgen import powerlaw_csr
from test_gpu_khop_labor import batch_graph  # noqa: F401  (fixture)
from test_gpu_link_seeds import big  # noqa: F401  (fixture)
from test_gpu_weighted_tables import weighted_graph  # noqa: F401  (fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GRID_CAP = V.GRID_CAP  # GGMS_DEBUG_GRID_CAP
N_ROWS = 13 * 256 + 65  # 3393: kernels whose workgroup takes 256 items per round (4 waves x 64 rows, or 256 lanes)
N_SEEDS = 3400           # leaf samplers: 13 x 256 + 72, the widest per-round unit among them (walk tile T = 256)
N_LONG = 14              # one item per workgroup round: 3 x 4 + 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as o
    return o


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, ops):
    """Sets the grid cap for one test and puts the default back."""
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(GRID_CAP, request.param)
    yield request.param
    lib().ggms_debug_set_knob(GRID_CAP, -1)
    assert ops.device_status() == 0


@pytest.fixture()
def cap3(ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(GRID_CAP, 3)
    yield 3
    lib().ggms_debug_set_knob(GRID_CAP, -1)
    assert ops.device_status() == 0


@pytest.fixture(scope="module")
def graphs(ops):
    """test_gpu_parity's `graphs`, the "mid" one only."""
    ip, ix = powerlaw_csr(**P.GRAPHS["mid"])
    return {"mid": (ip, ix, ops.DeviceGraph(P.dev(ip), P.dev(ix)))}


# ------------------------------------------------------------------------------------------------------ update_rows
# k_update_rows: a wave takes a tile of 64 rows, a workgroup 256 rows per round (update_rows.hip); dims 1, 2, 25 and 128
# are rows of one 4-byte chunk, one 8-byte chunk, 25 4-byte chunks and 32 16-byte chunks (V = 1, 2, 1, 4).
@pytest.mark.parametrize("dim", [1, 2, 25, 128])
@pytest.mark.parametrize("rule", UPD.RULES, ids=UPD.RULE_IDS)
def test_update_rows(ops, cap, rule, dim):
    UPD.run_case(ops, rule, 5000, dim, N_ROWS, seed=70 * dim + rule + cap, num_empty=40)
    # the device count ends in the middle of round 3 of 5 (cap 3: rounds of 768 rows); the rest of the bound is canary
    UPD.run_case(ops, rule, 5000, dim, 2 * 768 + 300 + 7, seed=71 * dim + rule + cap, bound=N_ROWS, num_empty=40)


# k_update_long_rows: one row of 8192 16-byte chunks per workgroup round
@pytest.mark.parametrize("rule", UPD.RULES, ids=UPD.RULE_IDS)
def test_update_long_rows(ops, cap, rule):
    UPD.run_case(ops, rule, 20, 32768, N_LONG, seed=5 + rule + cap, num_empty=2)


# ------------------------------------------------------------------------------------------------------ gathers
# k_gather_rows: a wave takes a tile of 64 index entries, a workgroup 256 entries per round (extract.hip); one (source,
# output) pair per family: converting float, FP8 decode, Q8ROW dequantise.
GATHER_PAIRS = [(F32, F16), (E4M3, F16), (Q8ROW, BF16)]


@pytest.mark.parametrize("dim", [20, 128])
@GH.pairs(None, *GATHER_PAIRS)
def test_gathers(ops, cap, pair, dim):
    fam = FAMILY[pair[0]]
    for scatter, dev_count, mask in [(False, False, GH.ALL_ONES), (True, False, GH.ALL_ONES), (False, True, GH.ALL_ONES),
                                     (True, True, 255)]:
        # dev_count: the bound is n + 37, so the count ends inside the last round
        GH.gather_case(ops, fam, *pair, dim, N_ROWS, scatter=scatter, dev_count=dev_count, mask=mask)


# k_gather_long_rows: one index entry (a row of 8192 chunks or more) per workgroup round; 14 entries into 8 rows
@GH.pairs(None, *GATHER_PAIRS)
def test_gather_long_rows(ops, cap, pair):
    fam = FAMILY[pair[0]]
    for scatter, dev_count in fam.long_calls:
        GH.gather_case(ops, fam, *pair, fam.long_dims[-1], N_LONG, scatter=scatter, dev_count=dev_count, rows=8)


# the fused gathers (256 entries per workgroup round): plain rows with miss / tier counters, device count below the
# bound (3430 / 3393), then extract_dynamic + publish (k_dynamic_publish: 256 nodes per workgroup round)
def test_extract_cached_tiered_dynamic(ops, cap):
    bound, n, dim = N_ROWS + 37, N_ROWS, 100
    DC.test_extract_cached_device_count(ops, 3, bound, n, dim, F32)
    DC.test_extract_tiered_device_count(ops, bound, n, dim, F32)
    DC.test_extract_dynamic_and_publish_device_count(ops, bound, n, dim, F32)
    # and the converting forms with their counters, through the harness
    t = FAMILY[E4M3].store(E4M3, "cached")
    GH.cached_case(ops, t, F16, 0.5, 3, n=N_ROWS)
    GH.tiered_case(ops, FAMILY[E4M3].store(E4M3, "tiered"), F16, 3, n=N_ROWS)


# ------------------------------------------------------------------------------------------------------ quantize_rows
# k_q8row_rows at dim 20: 5 chunks of 4 elements -> 8 lanes per row, 8 rows per wave, 32 rows per workgroup round (64
# if a base only allowed 2-element chunks): 13 x 64 + 7 rows.  k_q8row_long (dim 1032 > 1024): one row per wave, 4 per
# workgroup round: 13 x 4 + 3 rows.
@pytest.mark.parametrize("src", [np.float32, np.float16], ids=["F32", "F16"])
@pytest.mark.parametrize("dim,rows", [(20, 13 * 64 + 7), (Q.REG_DIM + 8, 13 * 4 + 3)])
def test_q8row(ops, cap, dim, rows, src):
    v = Q._q8row_rows(rows, dim, src, seed=dim + rows)
    got = ops.quantize_rows(torch.from_numpy(v).to(Q.DEV), ops.Q8ROW).cpu().numpy()
    want = cpu_q8row(v)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"dim {dim}: rows {bad[:8].tolist()} differ"


# k_encode_elems: a lane takes kElemU = 4 chunks of 4 f32 elements per round, a workgroup 256 x 16 = 4096 elements
def test_flat_encodes(ops, cap):
    n = 13 * 256 * 16 + 7
    v = (np.random.RandomState(cap).standard_normal(n) * 100).astype(np.float32).reshape(1, n)
    t = torch.from_numpy(v).to(Q.DEV)
    assert_fp8_bytes(Q._gpu_bytes(ops.quantize_rows(t, torch.float8_e4m3fn)), v, "F8E4M3", "flat f32 -> e4m3")
    assert_bits(tensor_bits(ops.quantize_rows(t, torch.bfloat16), BF16), from_f32(v, BF16), np.isnan(v), "flat f32 -> bf16",
                dt=BF16)


# ------------------------------------------------------------------------------------------------------ leaf samplers
# seeds per workgroup round: khop3 128 (a tile), khop0 64 (generate) and <= 16 (resolve), khop2 256 (a wave of 64 streams
# x 4 seeds), khop1 / weighted 256 (k_weighted_keys; the draw kernel's grid is the RNG map and is not capped), hash_dedup
# 16 (a one-wave workgroup serves 4 streams x 4 seeds; 12 workgroups at cap 3), khop_labor 4 (a wave per seed).
LEAVES = {"khop3": P.test_sample_khop3, "khop0": P.test_sample_khop0, "khop1": P.test_sample_khop1,
          "khop2": P.test_sample_khop2, "weighted": P.test_sample_weighted_khop,
          "weighted_prefix": P.test_sample_weighted_khop_prefix, "weighted_hash_dedup": P.test_sample_weighted_khop_hash_dedup}


@pytest.mark.parametrize("name,fanout", [("khop3", 10), ("khop3", 25), ("khop0", 10), ("khop0", 25), ("khop1", 10), ("khop2", 10),
                                         ("khop2", 64), ("weighted", 10), ("weighted_prefix", 10), ("weighted_hash_dedup", 10)])
def test_leaf_samplers(ops, cap, graphs, name, fanout):
    LEAVES[name](ops, graphs, "mid", N_SEEDS, fanout)


# khop1 beyond the one-workgroup sort (8192 seeds): k_sort_hist / k_sort_scatter take tiles of 2048 seeds per workgroup
# round: 13 x 2048 + 77
def test_khop1_multi_tile_sort(ops, cap, graphs):
    P.test_sample_khop1(ops, graphs, "mid", 13 * 2048 + 77, 2)


# k_walk_topk_emit: a tile of T seeds per workgroup round, T = 256, 128, 64 by (visits + K) per seed, and the SPILL form
# (more than 128 visits per seed, T = 64).  More tiles than workgroups: the ticketed forms with look-back.
# k_random_walk: `by` seeds per workgroup round (1 .. 64).
@pytest.mark.parametrize("n,wl,p,nw,K", [(N_SEEDS, 3, 0.5, 4, 5), (N_SEEDS, 6, 0.1, 6, 10), (N_SEEDS, 10, 0.1, 10, 20),
                                         (13 * 64 + 7, 2, 0.1, 70, 80)], ids=["T256", "T128", "T64", "spill"])
def test_random_walk(ops, cap, graphs, n, wl, p, nw, K):
    P.test_sample_random_walk(ops, graphs, "mid", n, wl, p, nw, K)


# k_labor_select: a wave per seed, 4 seeds per workgroup round, seed ids kept two rounds ahead; k_labor_hub: one hub list
# (more than kLaborWaveMax = 1024 neighbours) per workgroup round -- 14 hubs among 3386 ordinary seeds
def test_khop_labor(ops, cap):
    rng = np.random.RandomState(21)
    hubs = rng.permutation(N_SEEDS)[:N_LONG]
    deg = rng.randint(0, 120, N_SEEDS)
    deg[hubs] = rng.randint(LABOR.WAVE_MAX + 1, 3000, N_LONG)
    ip, ix = LABOR.graph_of_lists([rng.randint(0, LABOR.NUM_ID, d) for d in deg])
    g = ops.DeviceGraph(P.dev(ip), P.dev(ix))
    LABOR.check_leaf(ops, g, ip, ix, rng.permutation(N_SEEDS).astype(np.uint32), 10, 0x4329F67E)


# the hub lists (6000 neighbours): khop3 at its fanout limit, khop0 through its heavy-list kernel -- one workgroup for all
def test_hub_graph_one_workgroup(ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(GRID_CAP, 1)
    try:
        P.test_samplers_on_hub_graph(ops, "khop3", 127)
        P.test_samplers_on_hub_graph(ops, "khop0", 2048)
        P.test_samplers_on_hub_graph(ops, "khop0", 100)
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)
    assert ops.device_status() == 0


# ------------------------------------------------------------------------------------------------------ sample_batch
# 1000 seeds x [25, 10]: layers of 1000 and about 20 000 seeds (8 and 150 khop3 tiles, 20 scan tiles of 1024, 10 owner
# tiles of 2048); 1000 x [5, 10, 15]: 1000, about 5500 and 45 000.  Under the cap: the fused khop3 kernel's ticketed form,
# the owner scans with 1 or 3 chunks, the hashtable kernels and the single-pass scans' round loop.
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["khop3", "khop0", "khop2", "khop1"])
@pytest.mark.parametrize("fanouts,nseed", [([25, 10], 1000), ([5, 10, 15], 1000)], ids=["25-10", "5-10-15"])
def test_sample_batch(ops, cap, stype, fanouts, nseed, direct):
    P.test_sample_batch_vs_oracle(ops, stype, fanouts, nseed, direct)


@pytest.mark.parametrize("stype", ["weighted", "random_walk", "random_walk_long"])
def test_sample_batch_weighted_and_random_walk(ops, cap, stype):
    P.test_sample_batch_weighted_and_random_walk(ops, stype)


# the other sample types as batches of 1000 seeds, both tables: alias, prefix sums, hash_dedup (whose batch form enters its
# picks into the dedup table from inside the capped launch) and random walks, on tables built from weights
def _other_batch(ops, graph, stype, fanouts, direct):
    ip, ix, prob, alias, prefix = graph
    N = ip.size - 1
    g = ops.DeviceGraph(WT.dev(ip), WT.dev(ix))
    if stype == "weighted":
        code, ocode, kw, okw = ops.WEIGHTED_KHOP, oracle.WEIGHTED_KHOP, dict(prob_table=WT.dev(prob), alias_table=WT.dev(alias)), \
            dict(prob=prob, alias=alias)
    elif stype == "weighted_prefix":
        code, ocode, kw, okw = ops.WEIGHTED_KHOP_PREFIX, oracle.WEIGHTED_KHOP_PREFIX, dict(prob_table=WT.dev(prefix)), dict(prob=prefix)
    elif stype == "weighted_hash_dedup":
        code, ocode, kw, okw = ops.WEIGHTED_KHOP_HASH_DEDUP, oracle.WEIGHTED_KHOP_HASH_DEDUP, \
            dict(prob_table=WT.dev(prob), alias_table=WT.dev(alias)), dict(prob=prob, alias=alias)
    else:
        code, ocode = ops.RANDOM_WALK, oracle.RANDOM_WALK
        kw = dict(random_walk_length=3, random_walk_restart_prob=0.5, num_random_walk=4)
        okw = dict(walk_length=3, restart_prob=0.5, num_walk=4)
    bs = ops.BatchSampler(g, fanouts, 1000, sample_type=code, seed=5, direct_table=direct, **kw)
    st_orc = oracle.random_states(bs.states.shape[0], 5)
    rng = np.random.RandomState(len(fanouts))
    for rep in range(2):
        seeds = rng.permutation(N)[:1000].astype(np.uint32)
        if rep == 1:
            seeds[5] = seeds[0]  # a duplicated seed: local ids of raw seeds go through the table
        bs.sample(WT.dev(seeds))
        got, want = bs.result(), oracle.do_sample(ocode, ip, ix, seeds, fanouts, st_orc, **okw)
        WT.same_batch_as_oracle(got, want, len(fanouts), f"{stype} batch {rep}")
        if stype == "random_walk":
            for i in range(len(fanouts)):
                np.testing.assert_array_equal(WT.host_u32(got["layers"][i]["data"]), want["layers"][i]["data"])
        np.testing.assert_array_equal(bs.states.cpu().numpy().view(np.uint32), WT.wc.states_rows(st_orc))


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["weighted", "weighted_prefix", "weighted_hash_dedup", "random_walk"])
@pytest.mark.parametrize("fanouts", [[25, 10], [5, 10, 15]], ids=["25-10", "5-10-15"])
def test_sample_batch_other_types(ops, cap, weighted_graph, stype, fanouts, direct):  # noqa: F811
    _other_batch(ops, weighted_graph, stype, fanouts, direct)


# the suite's own batch check of the prefix and hash_dedup samplers (500 seeds, [10, 5]), both tables
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
@pytest.mark.parametrize("stype", ["prefix", "hash_dedup"])
def test_sample_batch_prefix_and_hash_dedup(ops, cap, weighted_graph, stype, direct):  # noqa: F811
    WT.test_sample_batch_prefix_and_hash_dedup(ops, weighted_graph, stype, direct)


# khop3 can no longer enter distinct seeds inside the first layer's launch (8 tiles, 1 or 3 workgroups): k_seed_enter +
# the ticketed layer kernel; batches 0 and 2 carry the promise, batch 1 does not
@pytest.mark.parametrize("stype", ["khop3", "khop0", "khop2", "khop1", "weighted", "random_walk"])
@pytest.mark.parametrize("fanouts,nseed", [([25, 10], 1000), ([5, 10, 15], 1000)], ids=["25-10", "5-10-15"])
def test_sample_batch_distinct_seeds(ops, cap, stype, fanouts, nseed):
    V.test_distinct_seed_promise_gives_the_oracles_batch(ops, stype, fanouts, nseed)


# k_seed_enter (khop3's distinct seeds outside the first layer's launch; the one small launch of the others): 256 seeds
# per workgroup round -- 1000 seeds are 2 rounds at cap 3, 3393 are 5
@pytest.mark.parametrize("stype", ["khop3", "khop1"])
def test_distinct_seeds_enter_over_four_rounds(ops, cap, stype):
    V.test_distinct_seed_promise_gives_the_oracles_batch(ops, stype, [4, 3], N_ROWS)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_sample_batch_khop_labor(ops, cap, batch_graph, direct):  # noqa: F811
    LABOR.test_batch_equals_the_reference_chain(ops, batch_graph, [15, 10, 5], direct)


# batches in flight on their own pipelines (streams, tables, workspaces): batch order on the RNG pool holds
def test_batches_in_flight(ops, cap):
    P.test_batches_in_flight_keep_batch_order(ops, "khop3")
    V.test_distinct_seed_batches_in_flight(ops)


# k_prefetch_list walks edge tiles (walk_edge_tiles, 2048 edges per workgroup round): a hub of 300 000 edges, 147 tiles
def test_prefetch_batch_sampler(cap3):
    A4.test_prefetch_sampler_equals_the_replay(A4.LEAF[3])


# ------------------------------------------------------------------------------------------------------ link prediction
# k_link_seeds: a wave per positive, 4 positives per workgroup round: 257 positives = 65 rounds' worth, 22 rounds at cap 3
@pytest.mark.parametrize("mode", [LINK.ref.UNIFORM, LINK.ref.EXCLUDE], ids=["uniform", "exclude"])
def test_link_seeds(ops, cap, big, mode):  # noqa: F811
    LINK.test_equals_the_reference(ops, big, 64, mode, 257)


# k_drop_snapshot / k_drop_compact: tiles of 1024 edges over ALL layers, one tile per workgroup round: 6 + 6 + 2 = 14.
# k_drop_build: 256 pairs per workgroup round: 3393 pairs (sources 0 .. 99, destinations 100 .. 199, repeats among them)
@pytest.mark.parametrize("which", [1, 3], ids=["self", "both"])
def test_drop_pair_edges(ops, cap, which):
    src, dst = DROP.make_pairs(N_ROWS)
    r0, c0 = DROP.big_layer(src, dst, seed=2)
    r1, c1 = DROP.big_layer(src, dst, seed=3)
    rng = np.random.RandomState(4)
    n2 = DROP.TILE + 77
    r2 = np.concatenate([dst[:40], rng.randint(0, 300, n2 - 40)]).astype(np.uint32)
    c2 = np.concatenate([src[:40], rng.randint(0, 300, n2 - 40)]).astype(np.uint32)
    want, dropped = DROP.run_and_check(ops, src, dst, which, [(r0, c0, DROP.BIG, DROP.BIG), (r1, c1, DROP.BIG, DROP.BIG),
                                                              (r2, c2, n2, n2)])
    assert all(0 < d for d in dropped)


# ------------------------------------------------------------------------------------------------------ closure
# k_closure_expand: edge tiles of 2048 per workgroup round (walk_edge_tiles); six lists of 6000 edges among the frontier's
# (18 tiles and more), and a frontier of 6000 nodes of which every 50th has a list (a tile spans many frontier nodes).
# k_closure_seeds: 2048 seeds per workgroup round: 13 x 2048 + 77 seeds, repeats among them.
def test_khop_closure(ops, cap):
    CLOSURE.test_closure_levels_equal_bfs(ops, "hub")
    CLOSURE.test_closure_frontier_with_long_runs_of_empty_lists(ops)
    ip, ix = CLOSURE.GRAPHS["hub"]()
    N = ip.size - 1
    seeds = np.random.RandomState(cap).randint(0, N, 13 * 2048 + 77)
    visit = torch.zeros(N, dtype=torch.int32, device="cuda")
    got = CLOSURE._closure_levels(ops, ops.DeviceGraph(CLOSURE._dev(ip), CLOSURE._dev(ix)), seeds, 1, visit, 1)
    for h, want in enumerate(CLOSURE.bfs_levels(ip, ix, seeds, 1)):
        np.testing.assert_array_equal(got[h], want, err_msg=f"hop {h}")


# ------------------------------------------------------------------------------------------------------ elementwise
# 256 items per workgroup round (k_count_nodes, the miss / hit split's scans of 1024, k_ht_insert, k_map_rest,
# k_map_edges); the owner split and the chunked owner scan give every workgroup one contiguous chunk instead
def test_count_nodes_and_cache_split(ops, cap):
    DC.test_count_nodes(ops, N_ROWS + 37, N_ROWS)
    DC.test_count_nodes(ops, 14_001, 14_001)
    P.test_get_miss_cache_index(ops, 14_001, 0.3)
    DC.test_get_miss_cache_index_dev(ops, 14_001 + 37, 14_001, 0.3)


def test_owner_split(ops, cap):
    OWNER.test_owner_split_mixed_table(ops, 14_001, 3)
    OWNER.test_owner_split_device_count(ops, 14_001 + 37, 14_001, 8)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hashed"])
def test_hashtable(ops, cap, direct):
    P.test_hashtable_fill_and_map(ops, 14_000, direct)  # fills of 14 000 and 28 000 items out of 7000 ids


# k_batch_handoff has one workgroup per 16 KiB and no round loop, so the cap leaves it alone: this case cannot reach a
# later round, it only guards that the hand-off and the queue's pack / unpack are untouched while the knob is set
def test_handoff_and_queue(cap3):
    A3.test_batch_handoff_leaf_against_numpy()
    A5.test_queue_pack_unpack_leaf_against_numpy()


# ------------------------------------------------------------------------------------------------------ scans
# the help path meets the round loop: tile / chunk 0's workgroup starts late (it also owns tiles 3, 6, ...), and patience 0
def test_scan_owner_of_tile_0_arrives_late(ops, cap3):
    SCAN.test_owner_of_the_first_chunk_arrives_after_the_total_is_out(ops, 60_000, False)
    SCAN.test_owner_of_the_first_chunk_arrives_after_the_total_is_out(ops, 5000, True)


def test_scan_patience_0(ops, cap3):
    from xgnn_amd import lib
    lib().ggms_debug_set_scan_patience(0)
    try:
        for direct in (True, False):
            P.test_sample_batch_vs_oracle(ops, "khop3", [25, 10], 1000, direct)
            P.test_sample_batch_vs_oracle(ops, "khop0", [5, 10, 15], 300, direct)
        P.test_sample_batch_weighted_and_random_walk(ops, "random_walk")
    finally:
        lib().ggms_debug_set_scan_patience(SCAN.session_patience())


# ------------------------------------------------------------------------------------------------------ no knob
# the kernels' own clamps: update_rows launches at most 512 workgroups (131 072 rows per round), the gather at most 256
# (65 536 entries per round): two whole rounds and a 65-row third one
@pytest.mark.parametrize("rule", UPD.RULES, ids=UPD.RULE_IDS)
def test_update_rows_natural_second_round(ops, rule):
    UPD.run_case(ops, rule, 300_000, 4, 2 * 131_072 + 65, seed=9 + rule, num_empty=100)


def test_gather_natural_second_round(ops):
    GH.gather_case(ops, FAMILY[E4M3], E4M3, F16, 20, 2 * 65_536 + 65)
