"""Inputs and checks shared by the host and GPU tests of what the weighted / with-replacement samplers MEAN
(tests/test_weighted_meaning_host.py, tests/test_gpu_weighted_tables.py, tests/test_oracle_python_twin.py): tables
built from weights by the dataset tools' rules instead of random ones, streams warmed past the seeding artefact of the
state pool, lists without `fanout` distinct candidates, and the edges of valid prefix sums.
numpy and the oracle only; the one torch helper imports torch when it is called."""
import functools
from types import SimpleNamespace

import numpy as np

import oracle

# the weights of the frequency tests: zeros (prob == 0 slots, plateaus in the prefix sums), a 400 : 1 spread, fractions
FREQ_M = 16384
FREQ_W = [0, 1, 1, 2, 3, 5, 8, 13, 0, 0, 21, 34, 1, 1, 1, 1, 100, 0.5, 0.25, 7, 7, 7, 0, 2]
FREQ_CALLS = 4
SIGMA = 5.0  # the bound of test_khop_labor_host.py

GIVEUP_FANOUTS = [5, 16, 17, 18, 33, 49]  # 17: the 65536-try round ends on the seed's last pick; 18/33/49: 2/3/4 rounds
GIVEUP_N = 400


def shared_list_graph(M, w_list):
    """Nodes 0 .. M-1 each own the same list of D = len(w_list) neighbours M .. M+D-1 (which have no neighbours), with
    the weights w_list.  -> indptr, indices, weights, prob / alias (the alias-table tool's), prefix (the prefix-sum
    tool's), p = w / sum(w) in float64 (zeros when every weight is 0), M, D."""
    w_list = np.asarray(w_list, np.float64)
    D = w_list.size
    indptr = np.concatenate([np.arange(M + 1, dtype=np.int64) * D, np.full(D, M * D, np.int64)]).astype(np.uint32)
    indices = np.tile(np.arange(M, M + D, dtype=np.uint32), M)
    weights = np.tile(w_list.astype(np.float32), M)
    prob, alias = oracle.create_alias_table(indptr, indices, weights)
    prefix = oracle.create_prob_prefix_table(indptr, weights)
    total = w_list.sum()
    p = w_list / total if total > 0 else np.zeros(D)
    return SimpleNamespace(indptr=indptr, indices=indices, weights=weights, prob=prob, alias=alias, prefix=prefix, p=p,
                           M=M, D=D, w=w_list)


@functools.lru_cache(maxsize=None)
def freq_graph():
    """The graph of the frequency tests (built once per process; nobody writes to it)."""
    g = shared_list_graph(FREQ_M, FREQ_W)
    for a in (g.indptr, g.indices, g.weights, g.prob, g.alias, g.prefix):
        a.flags.writeable = False
    return g


def warmed_states(n, seed, W=32):
    """oracle.random_states(n, seed) with every stream advanced by W draws.  Stream t is curand_init(seed + t, 0, 0):
    the first ~20 draws of neighbouring streams are correlated (test_neighbouring_streams_start_correlated), which a
    frequency count ACROSS streams would mistake for a biased sampler."""
    st = oracle.random_states(n, seed)
    if W:
        for t in range(int(n)):
            oracle.xorwow_draws(st[t:t + 1], W)
    return st


def states_tensor(st, device="cuda"):
    """An oracle state array as the int32 [n, 6] device tensor ops.random_states returns: d, v0 .. v4 per row."""
    import torch
    a = np.empty((st.size, 6), np.uint32)
    a[:, 0] = st["d"]
    a[:, 1:] = st["v"]
    return torch.from_numpy(a.view(np.int32)).to(device)


def states_rows(st):
    """The same [n, 6] layout on the host, for comparing with a downloaded pool."""
    a = np.empty((st.size, 6), np.uint32)
    a[:, 0] = st["d"]
    a[:, 1:] = st["v"]
    return a


def task_states(num_task):
    """Pool size of khop1 / weighted_khop / weighted_khop_prefix for num_task = num_input * fanout tasks."""
    return (min(num_task, 512 * 1024) + 255) // 256 * 256


def stream_states(num_input):
    """Pool size of weighted_khop_hash_dedup: 256 streams per 1024 seeds."""
    return max(1, (num_input + 1023) // 1024) * 256


# ------------------------------------------------------------------ frequencies
FREQ_CONFIGS = [("alias", 1), ("alias", 4), ("prefix", 1), ("prefix", 4), ("khop1", 1), ("khop1", 4), ("hash_dedup", 5)]


def freq_num_states(kind, fanout):
    return stream_states(FREQ_M) if kind == "hash_dedup" else task_states(FREQ_M * fanout)


def freq_oracle_call(kind, fanout, states):
    """One call of sampler `kind` on the frequency graph, seeds 0 .. M-1 in order, on the oracle."""
    g = freq_graph()
    inp = np.arange(g.M, dtype=np.uint32)
    if kind == "alias":
        return oracle.sample_weighted_khop(g.indptr, g.indices, g.prob, g.alias, inp, fanout, states)
    if kind == "prefix":
        return oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, inp, fanout, states)
    if kind == "khop1":
        return oracle.sample_khop1(g.indptr, g.indices, inp, fanout, states)
    return oracle.sample_weighted_khop_hash_dedup(g.indptr, g.indices, g.prob, g.alias, inp, fanout, states)


def freq_expected(kind):
    g = freq_graph()
    return np.full(g.D, 1.0 / g.D) if kind == "khop1" else g.p


def counted_draws(kind, fanout, src, dst, M, D):
    """The one raw draw per seed that a call's output still shows -> (its counts per neighbour, the counts of the whole
    output).  khop1 / alias / prefix: the LAST edge of each seed's run (the adjacent-duplicate rule never drops an entry
    whose successor has another src, so it is the seed's last task as drawn).  hash_dedup: the FIRST pick of each seed
    (the first accepted candidate is always new).  Seeds are 0 .. M-1 in order and every one has D > fanout neighbours."""
    src, dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
    assert dst.size and dst.min() >= M and dst.max() < M + D, "a neighbour outside the shared list"
    if kind == "hash_dedup":
        assert src.size == M * fanout and np.array_equal(src, np.repeat(np.arange(M), fanout))
        one = dst[::fanout]
    else:
        last = np.flatnonzero(np.append(src[1:] != src[:-1], True))
        assert np.array_equal(src[last], np.arange(M)), "every seed keeps at least its last task"
        one = dst[last]
    return np.bincount(one - M, minlength=D), np.bincount(dst - M, minlength=D)


def max_abs_z(counts, p, trials):
    """Largest |count - trials p| in binomial standard deviations over the categories with p > 0; a category with
    p == 0 must not occur at all."""
    counts, p = np.asarray(counts, np.float64), np.asarray(p, np.float64)
    assert counts.sum() == trials
    assert np.all(counts[p == 0] == 0), f"impossible categories drawn: {counts[p == 0]}"
    pos = p > 0
    z = (counts[pos] - trials * p[pos]) / np.sqrt(trials * p[pos] * (1.0 - p[pos]))
    return float(np.abs(z).max())


def check_frequencies(kind, fanout, outputs, label):
    """outputs: the (src, dst) of FREQ_CALLS consecutive calls.  Prints and returns the worst |z|; asserts the 5-sigma
    bound on the counted draws and, for the weighted samplers, that no zero-weight neighbour occurs anywhere."""
    g = freq_graph()
    counted, whole = np.zeros(g.D, np.int64), np.zeros(g.D, np.int64)
    for src, dst in outputs:
        c, w = counted_draws(kind, fanout, src, dst, g.M, g.D)
        counted += c
        whole += w
    trials = g.M * len(outputs)
    z = max_abs_z(counted, freq_expected(kind), trials)
    print(f"{label} {kind} fanout {fanout}: {trials} trials, max |z| {z:.2f}")
    assert z <= SIGMA
    if kind != "khop1":
        assert np.all(whole[g.w == 0] == 0), f"zero-weight neighbours in the output: {whole[g.w == 0]}"
    return z


# ---------------------------------------------------------------------- give-up
def giveup_graph(fanout):
    """400 nodes for weighted_khop_hash_dedup's termination rule (include/ggms.h: a seed that has drawn 65536 candidates
    takes every further one).  prob is 1 and alias 0 wherever nothing else is said -- valid, the acceptance draw lies in
    (0, 1] and `u > 1` never holds -- so a slot yields its own neighbour.
      node 0      fanout + 1 copies of one id: 1 distinct candidate
      node 1      ids 100 .. 100 + fanout - 2, then the first four again: fanout + 3 entries, fanout - 1 distinct
      node 2      fanout + 2 DISTINCT ids, of which the last three have prob 0 and an alias among the first fanout - 1;
                  slot 0 has prob 0.5 and the alias of slot 1: fanout - 1 candidates, only through the alias ids
      nodes 3 ..  0 to 119 distinct random ids (no give-up there, whatever the fanout)
    -> indptr, indices, prob, alias."""
    assert fanout >= 5
    rng = np.random.RandomState(1000 + fanout)
    lists = [np.full(fanout + 1, 7, np.uint32),
             np.concatenate([np.arange(100, 100 + fanout - 1), np.arange(100, 104)]).astype(np.uint32),
             np.concatenate([np.arange(200, 200 + fanout - 1), [300, 301, 302]]).astype(np.uint32)]
    for v in range(3, GIVEUP_N):
        lists.append(rng.permutation(GIVEUP_N)[:rng.randint(0, 120)].astype(np.uint32))
    indptr = np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.uint32)
    indices = np.concatenate(lists)
    prob = np.ones(indices.size, np.float32)
    alias = np.zeros(indices.size, np.uint32)
    o2 = int(indptr[2])
    prob[o2], alias[o2] = 0.5, 201
    prob[o2 + fanout - 1: o2 + fanout + 2] = 0.0
    alias[o2 + fanout - 1: o2 + fanout + 2] = [200, 202, 200 + fanout - 2]
    return indptr, indices, prob, alias


def giveup_seeds(fanout, variant="base"):
    """base: nodes 0, 1, 2 then 297 distinct others (300 seeds: stream t serves positions t and t + 256).
    after: 600 seeds, with four distinct lists longer than `fanout` at positions 256, 257, 512, 513 -- what streams 0
           and 1 serve after their give-up seed, so it depends on the state that seed leaves.
    pair: base with nodes 0 and 1 again at positions 16 and 17 (other streams: a table of their own)."""
    indptr = giveup_graph(fanout)[0]
    deg = np.diff(indptr.astype(np.int64))
    others = np.random.RandomState(7 + fanout).permutation(np.arange(3, GIVEUP_N))
    if variant == "base":
        return np.concatenate([[0, 1, 2], others[:297]]).astype(np.uint32)
    if variant == "pair":
        s = np.concatenate([[0, 1, 2], others[:297]]).astype(np.uint32)
        s[16], s[17] = 0, 1
        return s
    assert variant == "after"
    s = np.concatenate([[0, 1, 2], others, others[:200]]).astype(np.uint32)
    long_ = [int(v) for v in others if deg[v] > fanout][:4]
    assert len(long_) == 4
    for pos, v in zip((256, 257, 512, 513), long_):
        s[pos] = v
    return s


def check_giveup_output(fanout, seeds, indptr, src, dst):
    """Every seed returns min(deg, fanout) edges in seed order (the termination rule RETURNS); node 0 returns `fanout`
    copies of its one id; node 1 and node 2 return their fanout - 1 distinct candidates and one repeat."""
    deg = np.diff(indptr.astype(np.int64))
    want = np.minimum(deg[seeds], fanout)
    assert np.array_equal(np.asarray(src), np.repeat(seeds, want))
    off = np.concatenate([[0], np.cumsum(want)])
    dst = np.asarray(dst)
    for pos in np.flatnonzero(seeds <= 2):
        got = dst[off[pos]: off[pos + 1]]
        assert got.size == fanout
        if seeds[pos] == 0:
            assert np.all(got == 7)
        elif seeds[pos] == 1:
            assert set(got.tolist()) == set(range(100, 100 + fanout - 1))
        else:
            assert set(got.tolist()) == set(range(200, 200 + fanout - 1))
    if fanout <= 18:
        # ordinary lists: `fanout` DISTINCT picks.  Not claimed for 33 and 49: a probe sequence (triangular steps mod 50)
        # visits 26 of the 50 slots, and with more entries than that it can end on the OTHER documented bound -- 64
        # steps without a free slot or the value: the candidate is taken, possibly a second time
        for pos in np.flatnonzero((seeds > 2) & (deg[seeds] > fanout)):
            assert np.unique(dst[off[pos]: off[pos + 1]]).size == fanout


# ------------------------------------------------------------------ prefix edges
def prefix_edge_lists():
    """Weight lists at the edges of the prefix-sum search: lengths 1, 2, 3 (the `hi - lo >= 2` limit), zero weights
    (plateaus; a leading zero makes `x <= prefix[0]` false for every x > 0), a sum that stops growing in f32
    (2^24 + 1 == 2^24), an all-zero list, lengths around a power of two, a long list.  Integer weights: u * total can
    equal a prefix value exactly."""
    return [[1], [0, 1], [1, 0], [1, 1, 1], [0, 0, 5, 0, 0],
            [3, 0, 0, 0, 0, 0, 0, 2],
            [2 ** 24, 1, 1, 1, 1, 1, 1, 1],
            [0, 0, 0],
            [1] * 65,
            [0] * 30 + [4] + [0] * 33 + [1],
            [1, 2, 3, 4] * 300]


PREFIX_M = 512


def allowed_prefix_positions(w_list):
    """Positions of a list the prefix-sum sampler may return."""
    w = np.asarray(w_list, np.float64)
    if not w.any():
        return np.array([0])  # total 0: x == 0 <= prefix[0], the first branch
    if w[0] == 2 ** 24:
        return np.array([0])  # the f32 sums never leave 2^24: every x <= prefix[0]
    return np.flatnonzero(w > 0)


def check_prefix_output(w_list, dst, M):
    pos = np.unique(np.asarray(dst).astype(np.int64) - M)
    allowed = allowed_prefix_positions(w_list)
    assert np.all(np.isin(pos, allowed)), f"positions {pos[~np.isin(pos, allowed)]} drawn, weights {w_list[:12]}"
    if len(w_list) == 8 and w_list[0] == 3:
        assert set(pos.tolist()) == {0, 7}  # both ends occur, nothing between


# ------------------------------------------------------- x == a prefix value, exactly
TIE_W = [1] * 8


def tie_states(n):
    """Hand-made states whose FIRST draw makes u * total hit a prefix value of TIE_W exactly.  With v0 = v4 = 0 the
    xorshift word of the next draw is 0 and the draw is d + 362437; the draw k 2^29 - 1 (k = 1 .. 8; converted to f32 it
    is k 2^29) gives curand_uniform = k / 8 and x = k = prefix[k - 1], so stream t must return position t % 8: the
    interval of position j is (prefix[j - 1], prefix[j]].  A search that sends the tie upwards returns j + 1."""
    st = np.zeros(int(n), oracle.XORWOW_DTYPE)
    t = np.arange(int(n), dtype=np.uint64)
    k = t % np.uint64(8) + np.uint64(1)
    st["d"] = ((k << np.uint64(29)) - np.uint64(1) - np.uint64(362437)).astype(np.uint32)
    st["v"][:, 1] = (t * np.uint64(2654435761) + np.uint64(12345)).astype(np.uint32)  # what follows the first draw
    st["v"][:, 2] = (t * np.uint64(40503) + np.uint64(977)).astype(np.uint32)
    st["v"][:, 3] = (t * np.uint64(69069) + np.uint64(1)).astype(np.uint32)
    return st
