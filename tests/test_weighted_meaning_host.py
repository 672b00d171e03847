"""What the weighted / with-replacement samplers MEAN, on the oracle alone (no GPU): draw frequencies against
w / sum(w) in float64 from tables the dataset tools' rules build, the seeding artefact that makes those tests warm
their streams, and the termination rule of weighted_khop_hash_dedup (include/ggms.h) on lists without `fanout`
distinct candidates.  tests/test_gpu_weighted_tables.py runs the same inputs on the GPU; that they stay within their
bounds on the reference's reading alone is shown here."""
import time

import numpy as np
import pytest

import oracle
import weighted_cases as wc


@pytest.mark.parametrize("kind,fanout", wc.FREQ_CONFIGS)
def test_draw_frequencies_follow_the_weights(kind, fanout):
    """16384 seeds sharing one 24-neighbour list, 4 consecutive calls on warmed streams: 65536 counted draws.  Every
    neighbour within 5 binomial standard deviations of trials * w / sum(w) (1 / D for khop1); a zero-weight neighbour
    nowhere in the output.  A sampler that reads `r < prob` where it should read `r > prob` (hash_dedup), searches the
    prefix sums on the wrong side, or feeds the wrong draw to `% len` misses this by tens of sigma."""
    states = wc.warmed_states(wc.freq_num_states(kind, fanout), 2024)
    outs = [wc.freq_oracle_call(kind, fanout, states) for _ in range(wc.FREQ_CALLS)]
    wc.check_frequencies(kind, fanout, outs, "oracle")


def _chi_square_mod(draws, D):
    n = draws.size
    obs = np.bincount(draws % D, minlength=D).astype(np.float64)
    return float(((obs - n / D) ** 2 / (n / D)).sum())


@pytest.mark.parametrize("seed", [2024, 0x1001])
def test_neighbouring_streams_start_correlated(seed):
    """states[t] = curand_init(seed + t, 0, 0), as the reference seeds its pool: draw k of 16384 CONSECUTIVE streams is
    far from uniform mod 24 for small k (23 degrees of freedom: draw 2 gives a chi-square above 10000, residue 2 mod 4
    never occurs in draw 1) and unremarkable from draw 24 on.  The reference's behaviour, kept bit for bit; the reason
    the frequency tests skip 32 draws per stream."""
    n, K = 16384, 48
    st = oracle.random_states(n, seed)
    draws = np.stack([oracle.xorwow_draws(st[t:t + 1], K) for t in range(n)])
    chi = [_chi_square_mod(draws[:, k], 24) for k in range(K)]
    print("chi-square of draw k mod 24:", " ".join(f"{k}:{c:.0f}" for k, c in enumerate(chi)))
    assert chi[0] < 80          # draw 0 is fine
    assert chi[2] > 1000
    assert not np.any(draws[:, 1] % 4 == 2)
    assert max(chi[24:]) < 80


def test_frequencies_need_the_warm_up():
    """The same count on FRESH streams fails for the artefact's sake alone (khop1, fanout 1: tens of sigma)."""
    g = wc.freq_graph()
    states = wc.warmed_states(wc.freq_num_states("khop1", 1), 2024, W=0)
    counted = np.zeros(g.D, np.int64)
    for _ in range(wc.FREQ_CALLS):
        src, dst = wc.freq_oracle_call("khop1", 1, states)
        counted += wc.counted_draws("khop1", 1, src, dst, g.M, g.D)[0]
    z = wc.max_abs_z(counted, wc.freq_expected("khop1"), g.M * wc.FREQ_CALLS)
    print(f"khop1 fanout 1 on fresh streams: max |z| {z:.1f}")
    assert z > 20


@pytest.mark.parametrize("variant", ["base", "after", "pair"])
@pytest.mark.parametrize("fanout", wc.GIVEUP_FANOUTS)
def test_hash_dedup_gives_up_and_returns(fanout, variant):
    """Lists with fewer than `fanout` distinct candidates (the reference spins on them): every seed returns, node 0
    `fanout` copies of its one id, nodes 1 and 2 their fanout - 1 candidates and one repeat; twice, the second call
    from the states the first leaves."""
    indptr, indices, prob, alias = wc.giveup_graph(fanout)
    seeds = wc.giveup_seeds(fanout, variant)
    states = oracle.random_states(wc.stream_states(seeds.size), 0x1001)
    for rep in range(2):
        t0 = time.perf_counter()
        src, dst = oracle.sample_weighted_khop_hash_dedup(indptr, indices, prob, alias, seeds, fanout, states)
        dt = time.perf_counter() - t0
        wc.check_giveup_output(fanout, seeds, indptr, src, dst)
    print(f"fanout {fanout} {variant}: {dt * 1e3:.1f} ms")


def test_giveup_graph_is_what_it_says():
    for fanout in wc.GIVEUP_FANOUTS:
        indptr, indices, prob, alias = wc.giveup_graph(fanout)
        assert indptr.size == wc.GIVEUP_N + 1 and indices.max() < wc.GIVEUP_N
        l0, l1, l2 = (indices[indptr[v]: indptr[v + 1]] for v in range(3))
        assert l0.size == fanout + 1 and np.unique(l0).size == 1
        assert l1.size == fanout + 3 and np.unique(l1).size == fanout - 1
        assert l2.size == fanout + 2 and np.unique(l2).size == fanout + 2   # distinct by id ...
        p2, a2 = prob[indptr[2]: indptr[3]], alias[indptr[2]: indptr[3]]
        cand = set(l2[p2 > 0].tolist()) | set(a2[p2 < 1].tolist())          # ... fanout - 1 through the table
        assert len(cand) == fanout - 1 and np.count_nonzero(p2 == 0) == 3
        for v in range(3, wc.GIVEUP_N):
            lst = indices[indptr[v]: indptr[v + 1]]
            assert np.unique(lst).size == lst.size < 120
        for variant, n in (("base", 300), ("after", 600), ("pair", 300)):
            s = wc.giveup_seeds(fanout, variant)
            assert s.size == n and s[:3].tolist() == [0, 1, 2]
        assert np.unique(wc.giveup_seeds(fanout, "base")).size == 300


def test_prefix_edge_tables_are_what_they_say():
    """The edges the lists are there for exist in the tables the tool's rule builds."""
    lists = wc.prefix_edge_lists()
    tables = [wc.shared_list_graph(2, w).prefix[: len(w)] for w in lists]
    assert tables[6].tolist() == [2.0 ** 24] * 8                     # the f32 sum stops growing
    assert tables[7].tolist() == [0.0] * 3
    assert tables[5].tolist() == [3.0] * 7 + [5.0]                   # a plateau
    assert tables[9][:30].tolist() == [0.0] * 30 and tables[9][-1] == 5.0
    assert tables[10][-1] == 3000.0                                  # exact integers: ties with u * total can occur
    assert [len(w) for w in lists[:4]] == [1, 2, 2, 3]


def test_prefix_tie_goes_to_the_position_that_ends_there():
    """u * total == prefix[j] exactly (hand-made states: random draws meet such a tie about once in 2^14 even on the
    integer lists) selects position j, the one whose weight interval (prefix[j-1], prefix[j]] ends there."""
    g = wc.shared_list_graph(wc.PREFIX_M, wc.TIE_W)
    states = wc.tie_states(wc.task_states(g.M))
    u = oracle.xorwow_uniforms(states[3:4].copy(), 1)[0]
    assert u == np.float32(4 / 8)                                     # stream 3: k = 4
    src, dst = oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, np.arange(g.M, dtype=np.uint32), 1, states)
    assert np.array_equal(src, np.arange(g.M))
    assert np.array_equal(dst.astype(np.int64) - g.M, np.arange(g.M) % 8)


@pytest.mark.parametrize("fanout", [1, 3])
def test_prefix_edges_on_the_oracle(fanout):
    for w in wc.prefix_edge_lists():
        g = wc.shared_list_graph(wc.PREFIX_M, w)
        inp = np.arange(g.M, dtype=np.uint32)
        states = oracle.random_states(wc.task_states(g.M * fanout), 31)
        for rep in range(2):
            src, dst = oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, inp, fanout, states)
            wc.check_prefix_output(w, dst, g.M)
