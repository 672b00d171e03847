"""A second, independent restatement of the reference's sampling paths (khop3 + the layer loop, khop0, weighted_khop,
weighted_khop_prefix, weighted_khop_hash_dedup with the two bounds of include/ggms.h, khop1, random walk + top-K) --
plain Python loops written against the CUDA text,
not against oracle/ggms_oracle.c -- and the C oracle must agree with it on small cases.

What this adds: the oracle is one reading of racy CUDA code; this twin is the same canonical reading
(lock-step draw, first-occurrence dedup) restated from the sources a second time, structured like the kernels themselves
(blocks of 128 seeds, 8 groups, a 128-slot open-addressing set with triangular probing, the padded tmp arrays and their
compaction), so a slip in either restatement shows up as a difference.  It cannot pin the four curand_init constants
(both read tests/golden/xorwow_constants.json).

    sample_khop3 / _SetInsert        cuda/cuda_sampling_khop3.cu:51-146
    count_edge / compact_edge        :148-230 (keep entries whose src is not kEmptyKey, in (seed, slot) order)
    GPUSampleKHop3 launch geometry   :234-318 (GROUP_SIZE 16, BLOCK_WARP 8, TILE_SIZE 128; state i = 8 b + y)
    DoGPUSample layer loop           dist/dist_loops.cc:100-368
    OrderedHashTable contract        cuda/cuda_hashtable.cu:744-912 (contiguous local ids, prefix-stable; canonical:
                                     first occurrence owns the key)
    curand_init / curand             cuRAND XORWOW, constants of tests/golden/xorwow_constants.json
"""
import json
import os

import numpy as np
import pytest

import oracle
from graphgen import hub_csr, powerlaw_csr

EMPTY = 0xFFFFFFFF
M32 = 0xFFFFFFFF


class Xorwow:
    """curandStateXORWOW with subsequence = offset = 0."""

    def __init__(self, seed, const):
        c = const["curand_init_scramble"]
        b = const["base_state"]
        s0 = (seed & M32) ^ c["salt_lo"]
        s1 = ((seed >> 32) & M32) ^ c["salt_hi"]
        t0 = (c["mul_lo"] * s0) & M32
        t1 = (c["mul_hi"] * s1) & M32
        v = list(b["v"])
        self.v = [(v[0] + t0) & M32, v[1] ^ t0, (v[2] + t1) & M32, v[3] ^ t1, (v[4] + t0) & M32]
        self.d = (b["d"] + t1 + t0) & M32
        self.weyl = const["weyl_increment"]["value"]

    def next(self):
        v = self.v
        t = v[0] ^ (v[0] >> 2)
        v[0], v[1], v[2], v[3] = v[1], v[2], v[3], v[4]
        v[4] = (v[4] ^ ((v[4] << 4) & M32)) ^ (t ^ ((t << 1) & M32))
        self.d = (self.d + self.weyl) & M32
        return (v[4] + self.d) & M32


def khop3_twin(indptr, indices, inp, fanout, states):
    """sample_khop3 + count_edge + compact_edge.  states: list of Xorwow, advanced in place."""
    n = len(inp)
    tmp_src = [[EMPTY] * fanout for _ in range(n)]
    tmp_dst = [[EMPTY] * fanout for _ in range(n)]
    for b in range((n + 127) // 128):            # blockIdx.x
        for y in range(8):                       # threadIdx.y: one group of 16 lanes, one shared generator
            st = states[8 * b + y]
            table = [EMPTY] * 128                # DeviceSet.hashtable
            for index in range(128 * b + y, 128 * (b + 1), 8):
                if index >= n:
                    continue
                rid = int(inp[index])
                lo, hi = int(indptr[rid]), int(indptr[rid + 1])
                ln = hi - lo
                if ln <= fanout:
                    for j in range(ln):
                        tmp_src[index][j] = rid
                        tmp_dst[index][j] = int(indices[lo + j])
                    continue
                items = []                        # mark_pos: table positions in insertion order
                while len(items) < fanout:
                    rand = st.next() % ln         # the 16 lanes read one state: one draw per iteration
                    pos, offset = rand & 127, 1   # _SetInsert
                    while True:
                        if table[pos] == EMPTY:
                            table[pos] = rand
                            items.append(pos)
                            break
                        if table[pos] == rand:
                            break
                        pos = (pos + offset) & 127
                        offset += 1
                        assert offset < 128
                for j, p in enumerate(items):
                    tmp_src[index][j] = rid
                    tmp_dst[index][j] = int(indices[lo + table[p]])
                    table[p] = EMPTY              # "reset the hashtable values"
    src = [s for row in tmp_src for s in row if s != EMPTY]
    dst = [d for rs, rd in zip(tmp_src, tmp_dst) for s, d in zip(rs, rd) if s != EMPTY]
    return src, dst


def do_sample_twin(indptr, indices, seeds, fanouts, states):
    """DoGPUSample with khop3: layers from the last fanout to the first; the next layer's input is the table's
    unique list (seeds first, then every new node in first-occurrence order)."""
    local = {}                                    # OrderedHashTable: global id -> local id
    for s in seeds:                               # FillWithDupRevised(output_nodes)
        local.setdefault(int(s), len(local))
    cur = [int(s) for s in seeds]
    layers = [None] * len(fanouts)
    for i in range(len(fanouts) - 1, -1, -1):
        src, dst = khop3_twin(indptr, indices, cur, fanouts[i], states)
        for d in dst:                             # FillWithDuplicates(out_dst)
            local.setdefault(d, len(local))
        layers[i] = dict(col=[local[s] for s in src], row=[local[d] for d in dst],  # GPUMapEdges; col = new_src, row = new_dst
                         num_src=len(local), num_dst=len(cur))
        cur = list(local)                         # unique: insertion order of the dict = local id order
    return dict(layers=layers, input_nodes=cur)


def khop0_twin(indptr, indices, inp, fanout, const):
    """sample_khop0, NEW_ALGO (cuda/cuda_sampling_khop0.cu:102-153; launch :279-288: 32 lanes x 4 warps, 64 seeds per
    block).  Lane x of warp w of block b re-seeds its generator per launch from (b * 128 + x * 4 + w) + num_input and
    draws for the positions j >= fanout, j = x (mod 32), of the warp's seeds in turn: slot curand % (j + 1), taken if
    < fanout.  Colliding atomicExch on one slot resolve as if the positions came in ascending order (canonical:
    highest j wins).  Output compacted like khop3's."""
    n = len(inp)
    src, dst = [], []
    rows = [None] * n
    for b in range((n + 63) // 64):
        for w in range(4):
            lanes = [Xorwow(b * 128 + x * 4 + w + n, const) for x in range(32)]
            for index in range(64 * b + w, min(64 * (b + 1), n), 4):
                rid = int(inp[index])
                lo, hi = int(indptr[rid]), int(indptr[rid + 1])
                ln = hi - lo
                if ln <= fanout:
                    rows[index] = [int(indices[lo + j]) for j in range(ln)]
                    continue
                slots = [int(indices[lo + j]) for j in range(fanout)]
                for j in range(fanout, ln):        # ascending j: per lane its own order, across lanes highest j wins
                    k = lanes[j % 32].next() % (j + 1)
                    if k < fanout:
                        slots[k] = int(indices[lo + j])
                rows[index] = slots
    for index in range(n):
        for d in rows[index]:
            src.append(int(inp[index]))
            dst.append(d)
    return src, dst


def curand_uniform_twin(x):
    """curand_uniform: float(x) * 2^-32 + 2^-33, one rounding after the conversion of x (an fma in f32)."""
    xf = float(np.float32(x))                      # cvt.rn.f32.u32
    return np.float32(xf * 2.0 ** -32 + 2.0 ** -33)  # exact in f64 (24-bit factor), rounded once


def weighted_khop_twin(indptr, indices, prob, alias, inp, fanout, states):
    """sample_weighted_khop + stable SortPairs by src + count_edge / compact_edge
    (cuda/cuda_sampling_weighted_khop.cu:41-128, launch :156-181): task t -> seed t / fanout; thread t of a grid-stride
    launch over min(tasks, 512 K) threads rounded up to whole 256-thread blocks keeps generator t; a task takes TWO
    draws (position, acceptance); an entry equal to its successor after the sort is dropped (partial dedup by design)."""
    n = len(inp)
    num_task = n * fanout
    threads = min(num_task, 512 * 1024)             # Constant::kWeightedKHopMaxThreads, constant.h:72
    span = (threads + 255) // 256 * 256
    src = [EMPTY] * num_task
    dst = [0] * num_task
    for t in range(min(span, num_task)):
        st = states[t]
        for task in range(t, num_task, span):
            rid = int(inp[task // fanout])
            lo, hi = int(indptr[rid]), int(indptr[rid + 1])
            ln = hi - lo
            if ln == 0:
                continue                             # tmp_src = kEmptyKey, tmp_dst never written
            k = st.next() % ln
            r = curand_uniform_twin(st.next())
            src[task] = rid
            dst[task] = int(indices[lo + k]) if r < np.float32(prob[lo + k]) else int(alias[lo + k])
    order = sorted(range(num_task), key=lambda i: src[i])  # stable; kEmptyKey sorts last
    s_src, s_dst = [src[i] for i in order], [dst[i] for i in order]
    out_src, out_dst = [], []
    for i in range(num_task):
        if s_src[i] == EMPTY:
            continue
        if i + 1 < num_task and s_src[i] == s_src[i + 1] and s_dst[i] == s_dst[i + 1]:
            continue
        out_src.append(s_src[i])
        out_dst.append(s_dst[i])
    return out_src, out_dst


def random_walk_twin(indptr, indices, inp, walk_length, restart_prob, num_walk, K, states):
    """sample_random_walk (cuda/cuda_sampling_random_walk.cu:43-112; block shape :128-133: 256 threads reshaped to
    (bx, by) with bx halved while bx >= 2 * num_walk) + FrequencyHashmap::GetTopK's contract
    (cuda_frequency_hashmap.cu:643-841): per input POSITION the distinct visited nodes with their visit counts, the K
    most visited first, ties in first-visit order (canonical reading of the racy `index` field: the smallest position
    of the padded visit array), positions in input order; data = the count."""
    n = len(inp)
    bx, by = 256, 1
    while bx >= 2 * num_walk:
        bx //= 2
        by *= 2
    per = num_walk * walk_length
    visits = [[None] * per for _ in range(n)]       # tmp_dst by (position, step * num_walk + walk); None = kEmptyKey src
    for b in range((n + by - 1) // by):
        for x in range(bx):
            for y in range(by):
                node_idx = b * by + y
                if node_idx >= n:
                    continue
                st = states[256 * b + by * x + y]
                start = int(inp[node_idx])
                for walk in range(x, num_walk, bx):
                    node = start
                    for step in range(walk_length):
                        if node is None:
                            continue
                        lo, hi = int(indptr[node]), int(indptr[node + 1])
                        if hi == lo:
                            node = None
                            continue
                        k = st.next() % (hi - lo)
                        node = int(indices[lo + k])
                        visits[node_idx][step * num_walk + walk] = node
                        xx, yy = st.next(), st.next()  # curand_uniform_double: two draws, 53 bits
                        z = xx ^ (yy << 21)
                        if z * 2.0 ** -53 + 2.0 ** -54 < restart_prob:
                            node = None
    src, dst, data = [], [], []
    for node_idx in range(n):
        first, count = {}, {}
        for p, v in enumerate(visits[node_idx]):
            if v is None:
                continue
            first.setdefault(v, p)
            count[v] = count.get(v, 0) + 1
        order = sorted(first, key=lambda v: first[v])          # first-visit order ...
        order = sorted(order, key=lambda v: -count[v])[:K]     # ... kept among equal counts (stable sort, descending)
        for v in order:
            src.append(int(inp[node_idx]))
            dst.append(v)
            data.append(count[v])
    return src, dst, data


def _task_streams(num_task):
    """Threads of the task-per-thread launches (khop1.cu:153-156, weighted_khop_prefix.cu:172-175): min(tasks, 512 K)
    rounded up to whole blocks of 256; thread t keeps generator t and takes tasks t, t + span, ..."""
    return (min(num_task, 512 * 1024) + 255) // 256 * 256


def _sort_and_drop_adjacent(src, dst):
    """SortPairs by src (stable: an LSD radix sort) and count_edge / compact_edge as khop1.cu:74-126 and
    weighted_khop_prefix.cu:94-144 have them: entry i stays unless its src is kEmptyKey or (src, dst) equals entry
    i + 1's; the last entry stays unless empty."""
    n = len(src)
    order = sorted(range(n), key=lambda i: src[i])
    s, d = [src[i] for i in order], [dst[i] for i in order]
    keep = [s[i] != EMPTY and (i == n - 1 or s[i] != s[i + 1] or d[i] != d[i + 1]) for i in range(n)]
    return [s[i] for i in range(n) if keep[i]], [d[i] for i in range(n) if keep[i]]


def khop1_twin(indptr, indices, inp, fanout, states):
    """sample_khop1 (cuda/cuda_sampling_khop1.cu:42-72): task t -> seed t / fanout, ONE draw, neighbour curand % len;
    a seed without neighbours leaves kEmptyKey and takes no draw."""
    num_task = len(inp) * fanout
    span = _task_streams(num_task)
    src, dst = [EMPTY] * num_task, [EMPTY] * num_task
    for t in range(min(span, num_task)):
        for task in range(t, num_task, span):
            rid = int(inp[task // fanout])
            lo, ln = int(indptr[rid]), int(indptr[rid + 1]) - int(indptr[rid])
            if ln:
                src[task], dst[task] = rid, int(indices[lo + states[t].next() % ln])
    return _sort_and_drop_adjacent(src, dst)


def weighted_khop_prefix_twin(indptr, indices, prefix, inp, fanout, states):
    """sample_weighted_khop_prefix (cuda/cuda_sampling_weighted_khop_prefix.cu:41-92): ONE curand_uniform per task,
    scaled IN FLOAT by the list's last prefix sum; `x <= prefix[first]` takes the first neighbour, otherwise the
    bracket (low, high] = (first, last] is halved while it spans two or more, `prefix[mid] >= x` moving high, and the
    neighbour at `high` is taken."""
    f32 = np.float32
    num_task = len(inp) * fanout
    span = _task_streams(num_task)
    src, dst = [EMPTY] * num_task, [EMPTY] * num_task
    for t in range(min(span, num_task)):
        for task in range(t, num_task, span):
            rid = int(inp[task // fanout])
            lo, ln = int(indptr[rid]), int(indptr[rid + 1]) - int(indptr[rid])
            if ln == 0:
                continue
            x = f32(curand_uniform_twin(states[t].next()) * f32(prefix[lo + ln - 1]))   # f32 * f32, rounded once
            if x <= f32(prefix[lo]):
                pick = lo
            else:
                low, high = lo, lo + ln - 1
                while high - low >= 2:
                    mid = (low + high) >> 1
                    if f32(prefix[mid]) >= x:
                        high = mid
                    else:
                        low = mid
                pick = high
            src[task], dst[task] = rid, int(indices[pick])
    return _sort_and_drop_adjacent(src, dst)


def weighted_khop_hash_dedup_twin(indptr, indices, prob, alias, inp, fanout, states):
    """sample_weighted_khop_hash_dedup + insert_hash_table + count_edge / compact_edge
    (cuda/cuda_sampling_weighted_khop_hash_dedup.cu:41-115, launch :212-231: blocks of 256 threads over tiles of 1024
    seeds; thread t of block b keeps generator 256 b + t and walks seeds 1024 b + t + 256 r).  The thread's 50 slots
    {value, round} are set to kEmptyKey once per launch and never cleared between seeds: a slot is free for a seed when
    its round is not the seed's ID, so an earlier seed of the thread with the same id still counts.  A candidate is
    two draws: position curand % len, then curand_uniform u, the alias taken when u > prob (STRICTLY greater; the plain
    sampler takes the neighbour when u < prob).
    The two bounds include/ggms.h adds where the reference would spin: a probe walk ends after 64 steps and the candidate
    is taken (nothing stored); a seed that has drawn 65536 candidates takes every further one, new or not."""
    n = len(inp)
    rows = [None] * n
    for b in range((n + 1023) // 1024):
        for t in range(256):
            st = states[256 * b + t]
            value, round_ = [EMPTY] * 50, [EMPTY] * 50
            for index in range(1024 * b + t, min(1024 * (b + 1), n), 256):
                rid = int(inp[index])
                lo, ln = int(indptr[rid]), int(indptr[rid + 1]) - int(indptr[rid])
                if ln <= fanout:
                    rows[index] = [int(indices[lo + j]) for j in range(ln)]
                    continue
                picks, drawn = [], 0
                while len(picks) < fanout:
                    k = st.next() % ln
                    u = curand_uniform_twin(st.next())
                    drawn += 1
                    cand = int(alias[lo + k]) if u > np.float32(prob[lo + k]) else int(indices[lo + k])
                    pos, gap, new = cand % 50, 1, True
                    for _ in range(64):
                        if round_[pos] != rid:
                            round_[pos], value[pos] = rid, cand
                            break
                        if value[pos] == cand:
                            new = False
                            break
                        pos = (pos + gap) % 50
                        gap += 1
                    if new or drawn > 65536:
                        picks.append(cand)
                rows[index] = picks
    src = [int(inp[i]) for i in range(n) for _ in rows[i]]
    dst = [d for i in range(n) for d in rows[i]]
    return src, dst


@pytest.fixture(scope="module")
def const(golden_dir):
    return json.load(open(os.path.join(golden_dir, "xorwow_constants.json")))


def test_xorwow_twin_matches_the_oracle_stream(const):
    for seed in (0, 1, 0x5EED, (7 << 32) | 123):
        st = Xorwow(seed, const)
        want = oracle.xorwow_stream(seed, 200)
        assert [st.next() for _ in range(200)] == want.tolist()


@pytest.mark.parametrize("gname,nseed,fanouts,seed", [
    ("powerlaw", 300, [5, 4], 11),          # two blocks of 128 + a ragged third, short and long lists mixed
    ("powerlaw", 97, [3, 7, 5], 2),         # three layers, frontier grows past one block
    ("hub", 150, [25, 10], 5),              # 6000-neighbour lists: long rejection runs, probing in the 128-slot set
    ("hub", 40, [100], 9),                  # fanout near the set's capacity (< 128)
    ("powerlaw", 64, [1], 3),               # fanout 1
])
def test_c_oracle_agrees_with_the_python_twin(const, gname, nseed, fanouts, seed):
    ip, ix = powerlaw_csr(2500, mean_deg=12, seed=4) if gname == "powerlaw" else hub_csr()
    rng = np.random.RandomState(seed)
    seeds = rng.randint(0, ip.size - 1, nseed).astype(np.uint32)  # repeated seeds allowed, as in a raw batch
    nstates = 8 * 64
    orc_states = oracle.random_states(nstates, seed)
    twin_states = [Xorwow(seed + t, const) for t in range(nstates)]  # curand_init(seed + tid, 0, 0), cuda_random_states.cu:44
    want = do_sample_twin(ip, ix, seeds, fanouts, twin_states)
    got = oracle.do_sample(oracle.KHOP3, ip, ix, seeds, fanouts, orc_states)
    assert got["input_nodes"].tolist() == want["input_nodes"]
    for i in range(len(fanouts)):
        assert got["layers"][i]["row"].tolist() == want["layers"][i]["row"], f"layer {i} row"
        assert got["layers"][i]["col"].tolist() == want["layers"][i]["col"], f"layer {i} col"
        assert (got["layers"][i]["num_src"], got["layers"][i]["num_dst"]) == (want["layers"][i]["num_src"], want["layers"][i]["num_dst"])
    # the generators end where the twin's do: same number of draws per stream
    for t in range(nstates):
        assert int(orc_states["d"][t]) == twin_states[t].d and orc_states["v"][t].tolist() == twin_states[t].v


@pytest.mark.parametrize("gname,n,fanout", [("powerlaw", 333, 5), ("powerlaw", 64, 1), ("hub", 200, 25), ("hub", 70, 300)])
def test_c_oracle_khop0_agrees_with_the_python_twin(const, gname, n, fanout):
    ip, ix = powerlaw_csr(2500, mean_deg=12, seed=4) if gname == "powerlaw" else hub_csr()
    inp = np.random.RandomState(fanout).permutation(ip.size - 1)[:n].astype(np.uint32)
    want_src, want_dst = khop0_twin(ip, ix, inp, fanout, const)
    got_src, got_dst = oracle.sample_khop0(ip, ix, inp, fanout)
    assert got_src.tolist() == want_src and got_dst.tolist() == want_dst


@pytest.mark.parametrize("n,fanout,seed", [(200, 5, 1), (77, 12, 2), (3000, 3, 3)])
def test_c_oracle_weighted_khop_agrees_with_the_python_twin(const, n, fanout, seed):
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(1500, mean_deg=9, seed=6)            # includes nodes without neighbours
    w = np.random.RandomState(seed).randint(1, 11, ix.size).astype(np.float32)
    prob, alias = datagen.build_alias_tables(ip, ix, w, num_threads=2)
    inp = np.random.RandomState(seed + 10).randint(0, ip.size - 1, n).astype(np.uint32)  # repeated seeds allowed
    nstates = min(n * fanout, 512 * 1024)
    nstates = (nstates + 255) // 256 * 256
    orc_states = oracle.random_states(nstates, seed)
    twin_states = [Xorwow(seed + t, const) for t in range(nstates)]
    want_src, want_dst = weighted_khop_twin(ip, ix, prob, alias, inp, fanout, twin_states)
    got_src, got_dst = oracle.sample_weighted_khop(ip, ix, prob, alias, inp, fanout, orc_states)
    assert got_src.tolist() == want_src and got_dst.tolist() == want_dst
    for t in range(0, nstates, 7):
        assert int(orc_states["d"][t]) == twin_states[t].d and orc_states["v"][t].tolist() == twin_states[t].v


def test_curand_uniform_twin_against_the_oracle(const):
    xs = [0, 1, 2, 0xFFFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, 0x80000000, 0x7FFFFFFF, 123456789, 0x01000001, 0x00FFFFFF]
    got = [float(curand_uniform_twin(x)) for x in xs]
    assert all(0.0 < g <= 1.0 for g in got)
    assert got[0] == 2.0 ** -33 and got[3] == 1.0  # the open-closed interval of cuRAND: (0, 1]


@pytest.mark.parametrize("n,wl,p,nw,K,seed", [(150, 3, 0.5, 4, 5, 1), (70, 4, 0.2, 3, 2, 2), (33, 2, 0.0, 9, 10, 3), (40, 3, 0.5, 130, 5, 4)])
def test_c_oracle_random_walk_agrees_with_the_python_twin(const, n, wl, p, nw, K, seed):
    ip, ix = powerlaw_csr(1200, mean_deg=7, seed=8)            # includes nodes without neighbours (walks that die)
    inp = np.random.RandomState(seed).randint(0, ip.size - 1, n).astype(np.uint32)  # repeated positions are separate
    bx, by = 256, 1
    while bx >= 2 * nw:
        bx //= 2
        by *= 2
    nstates = (n + by - 1) // by * 256
    orc_states = oracle.random_states(nstates, seed)
    twin_states = [Xorwow(seed + t, const) for t in range(nstates)]
    want = random_walk_twin(ip, ix, inp, wl, p, nw, K, twin_states)
    got = oracle.sample_random_walk(ip, ix, inp, wl, p, nw, K, orc_states)
    assert [a.tolist() for a in got] == [list(w) for w in want]
    for t in range(0, nstates, 5):
        assert int(orc_states["d"][t]) == twin_states[t].d and orc_states["v"][t].tolist() == twin_states[t].v


# ---------------------------------------------- weighted_khop_prefix, weighted_khop_hash_dedup, khop1
def _twin_states(orc_states, const):
    """Twin generators in the states of an oracle pool (fresh, warmed or hand-made)."""
    out = []
    for s in orc_states:
        x = Xorwow.__new__(Xorwow)
        x.d, x.v, x.weyl = int(s["d"]), [int(w) for w in s["v"]], const["weyl_increment"]["value"]
        out.append(x)
    return out


def _assert_same_states(orc_states, twin_states):
    for t in range(len(twin_states)):
        assert int(orc_states["d"][t]) == twin_states[t].d and orc_states["v"][t].tolist() == twin_states[t].v, f"stream {t}"


def _weighted_powerlaw(seed):
    ip, ix = powerlaw_csr(1500, mean_deg=9, seed=6)            # includes nodes without neighbours
    w = np.random.RandomState(seed).randint(1, 11, ix.size).astype(np.float32)
    return ip, ix, w


@pytest.mark.parametrize("n,fanout,seed", [(200, 5, 1), (77, 12, 2), (3000, 3, 3), (64, 1, 4)])
def test_c_oracle_khop1_agrees_with_the_python_twin(const, n, fanout, seed):
    ip, ix, _ = _weighted_powerlaw(seed)
    inp = np.random.RandomState(seed + 10).randint(0, ip.size - 1, n).astype(np.uint32)  # repeated seeds allowed
    orc_states = oracle.random_states(_task_streams(n * fanout), seed)
    twin_states = _twin_states(orc_states, const)
    want = khop1_twin(ip, ix, inp, fanout, twin_states)
    got = oracle.sample_khop1(ip, ix, inp, fanout, orc_states)
    assert [a.tolist() for a in got] == [list(w) for w in want]
    _assert_same_states(orc_states, twin_states)


@pytest.mark.parametrize("n,fanout,seed", [(200, 5, 1), (77, 12, 2), (3000, 3, 3), (64, 1, 4)])
def test_c_oracle_weighted_khop_prefix_agrees_with_the_python_twin(const, n, fanout, seed):
    ip, ix, w = _weighted_powerlaw(seed)
    pre = oracle.create_prob_prefix_table(ip, w)
    inp = np.random.RandomState(seed + 10).randint(0, ip.size - 1, n).astype(np.uint32)
    orc_states = oracle.random_states(_task_streams(n * fanout), seed)
    twin_states = _twin_states(orc_states, const)
    want = weighted_khop_prefix_twin(ip, ix, pre, inp, fanout, twin_states)
    got = oracle.sample_weighted_khop_prefix(ip, ix, pre, inp, fanout, orc_states)
    assert [a.tolist() for a in got] == [list(w_) for w_ in want]
    _assert_same_states(orc_states, twin_states)


@pytest.mark.parametrize("fanout", [1, 3])
def test_c_oracle_weighted_khop_prefix_agrees_with_the_python_twin_on_table_edges(const, fanout):
    """Lengths 1 - 3, zero weights, a sum that stops growing, an all-zero list (weighted_cases.prefix_edge_lists), and
    u * total equal to a prefix value exactly (hand-made states)."""
    import weighted_cases as wc
    cases = [(w, None) for w in wc.prefix_edge_lists()] + [(wc.TIE_W, "tie")]
    for w, how in cases:
        g = wc.shared_list_graph(64, w)
        inp = np.arange(g.M, dtype=np.uint32)
        n = _task_streams(g.M * fanout)
        orc_states = wc.tie_states(n) if how else oracle.random_states(n, 31)
        twin_states = _twin_states(orc_states, const)
        want = weighted_khop_prefix_twin(g.indptr, g.indices, g.prefix, inp, fanout, twin_states)
        got = oracle.sample_weighted_khop_prefix(g.indptr, g.indices, g.prefix, inp, fanout, orc_states)
        assert [a.tolist() for a in got] == [list(w_) for w_ in want], w[:10]
        _assert_same_states(orc_states, twin_states)


@pytest.mark.parametrize("n,fanout,seed", [(300, 5, 1), (1100, 30, 2), (1025, 49, 3)])
def test_c_oracle_weighted_khop_hash_dedup_agrees_with_the_python_twin(const, n, fanout, seed):
    """Alias tables from weights; one stream meets the longest list three times (positions 0, 256, 512): its table
    still holds the earlier copies' entries, and from fanout 25 on it fills up (the 64-step probe bound)."""
    ip, ix, w = _weighted_powerlaw(seed)
    prob, alias = oracle.create_alias_table(ip, ix, w)
    inp = np.random.RandomState(seed + 10).randint(0, ip.size - 1, n).astype(np.uint32)
    if n > 512:
        inp[[0, 256, 512]] = int(np.argmax(np.diff(ip.astype(np.int64))))
    orc_states = oracle.random_states((n + 1023) // 1024 * 256, seed)
    twin_states = _twin_states(orc_states, const)
    want = weighted_khop_hash_dedup_twin(ip, ix, prob, alias, inp, fanout, twin_states)
    got = oracle.sample_weighted_khop_hash_dedup(ip, ix, prob, alias, inp, fanout, orc_states)
    assert [a.tolist() for a in got] == [list(w_) for w_ in want]
    _assert_same_states(orc_states, twin_states)


@pytest.mark.parametrize("fanout,variant", [(5, "base"), (17, "after"), (18, "pair")])
def test_c_oracle_hash_dedup_give_up_agrees_with_the_python_twin(const, fanout, variant):
    """Lists without `fanout` distinct candidates: both restatements stop rejecting after the same candidate (65536
    drawn), so the picks AND the generators agree -- one candidate earlier or later shifts every later draw of the
    stream.  17: the seed completes on candidate 65552; 18: it needs 65553; `after`: the stream serves two more long
    lists from the state the give-up seed leaves."""
    import weighted_cases as wc
    ip, ix, prob, alias = wc.giveup_graph(fanout)
    inp = wc.giveup_seeds(fanout, variant)
    orc_states = oracle.random_states(wc.stream_states(inp.size), 0x1001)
    twin_states = _twin_states(orc_states, const)
    want = weighted_khop_hash_dedup_twin(ip, ix, prob, alias, inp, fanout, twin_states)
    got = oracle.sample_weighted_khop_hash_dedup(ip, ix, prob, alias, inp, fanout, orc_states)
    assert [a.tolist() for a in got] == [list(w_) for w_ in want]
    _assert_same_states(orc_states, twin_states)
