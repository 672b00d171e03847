"""The dedup patterns of dedup_cases.py are what their names say (a typo in a generator must not quietly turn an edge
case into a random one), the numpy reference agrees with two independent restatements (a dict loop, oracle.HashTable),
and the comparator the GPU tests use rejects the wrong outputs a broken dedup would give.  No GPU."""
import numpy as np
import pytest

import dedup_cases as D
import oracle
from dedup_cases import CASES, FULL, TILE


def _owners(fills):
    """per fill: bool per instance -- it is the first occurrence of its key over everything entered so far"""
    seen, out = set(), []
    for a in fills:
        own = np.zeros(a.size, bool)
        for i, k in enumerate(a.tolist()):
            if k not in seen:
                seen.add(k)
                own[i] = True
        out.append(own)
    return out


def _per_chunk(own, items):
    return [int(own[s:s + items].sum()) for s in range(0, own.size, items)]


def test_the_constants_are_the_kernels():
    """dedup_cases.py restates the owner scan's tiling; hold it against the source it was read from."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xgnn_amd", "csrc", "hashtable.hip")).read()
    assert re.search(r"kOwnItems = 8, kOwnTile = kOwnItems \* kBlock;", src) and D.TILE == 8 * 256
    assert re.search(r"kChunkMaxTiles = 65535u / kOwnTile;", src) and D.CHUNK_MAX_TILES == 65535 // D.TILE == 31
    assert re.search(r"kOwnRounds = kOwnTile / \(2 \* kBlock\);", src) and D.ROUND == 2 * 256 and D.SEGMENT == D.ROUND // 4
    assert re.search(r"kChunkRegTiles = 2;", src)
    assert FULL == 63488


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 100_000])
def test_all_same(n):
    c = CASES[f"all_same-{n}"]
    assert [f.size for f in c.fills] == [n, n, n]
    assert [np.unique(f).size for f in c.fills] == [1, 1, 1]
    assert c.fills[0][0] == c.fills[1][0] != c.fills[2][0]
    own = _owners(c.fills)
    assert [int(o.sum()) for o in own] == [1, 0, 1] and own[0][0] and own[2][0]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("extra", [0, 1])
def test_all_distinct_full_chunks(k, extra):
    c = CASES[f"all_distinct_full_chunks-{k}" + ("-plus1" if extra else "")]
    n = k * FULL + extra
    assert c.chunks == k and [f.size for f in c.fills] == [n, n, n]
    own = _owners(c.fills)
    # with k workgroups a chunk is ceil(tiles / k) tiles: exactly kChunkMaxTiles when extra == 0 (one more tile does not
    # fit the 16-bit count: chunk_fits is false and the tile-chained kernel runs)
    tiles = (n + TILE - 1) // TILE
    per = (tiles + k - 1) // k
    assert (per == D.CHUNK_MAX_TILES) == (extra == 0) and (tiles <= D.CHUNK_MAX_TILES * k) == (extra == 0)
    assert _per_chunk(own[0], FULL)[:k] == [FULL] * k            # fill 1: every chunk is made of owners only
    assert own[0].all() and np.array_equal(np.sort(c.fills[0]), np.arange(n))
    assert not own[1].any() and np.array_equal(c.fills[0], c.fills[1])  # fill 2: every chunk carries 0
    assert np.array_equal(c.fills[2][:n - TILE], c.fills[0][::-1][:n - TILE])  # fill 3: reversed ...
    assert not own[2][:n - TILE].any() and own[2][n - TILE:].all()              # ... fresh ids in the last tile only
    if extra == 0:
        assert _per_chunk(own[2], FULL) == [0] * (k - 1) + [TILE]
    assert int(c.fills[2].max()) < c.num_node


def test_all_distinct_register_chunks():
    c = CASES["all_distinct_register_chunks"]
    n = c.fills[0].size
    assert c.chunks == 3 and n == 3 * 2 * TILE  # 6 tiles over 3 workgroups: two tiles per chunk = kChunkRegTiles
    own = _owners(c.fills)
    assert _per_chunk(own[0], 2 * TILE) == [2 * TILE] * 3   # every chunk fills the 4096-key LDS buffer
    assert _per_chunk(own[1], 2 * TILE) == [0] * 3
    assert _per_chunk(own[2], 2 * TILE) == [0, 0, TILE] and own[2][n - TILE:].all()


@pytest.mark.parametrize("chunks", [None, 3, 4])
def test_boundary_pairs(chunks):
    c = CASES["boundary_pairs" + (f"-chunks{chunks}" if chunks else "")]
    a = c.fills[0]
    n = a.size
    assert n % 2 == 1 and c.chunks == chunks
    per, nchunks, bounds = c.marks["per"], c.marks["nchunks"], c.marks["bounds"]
    assert per == {None: 1, 3: 2, 4: 3}[chunks] and (nchunks - 1) * per * TILE < n <= nchunks * per * TILE
    assert {128, 512, 2048, 2 * 2048, per * TILE, (nchunks - 1) * per * TILE} == set(bounds)
    for b in bounds:
        assert a[b - 1] == a[b], b
    assert a[0] == a[n - 1]
    # nothing else repeats: one instance lost per pair
    assert np.unique(a).size == n - len(bounds) - 1
    own = _owners(c.fills)[0]
    assert sorted(np.flatnonzero(~own).tolist()) == sorted(bounds + [n - 1])


def test_mirrored():
    a = CASES["mirrored"].fills[0]
    n = a.size
    assert n % 2 == 0 and np.array_equal(a, a[::-1])
    keys, counts = np.unique(a, return_counts=True)
    assert keys.size == n // 2 and (counts == 2).all()
    own = _owners([a])[0]
    assert own[:n // 2].all() and not own[n // 2:].any()
    assert n // 2 % TILE != 0  # the half does not end on a tile boundary


@pytest.mark.parametrize("m", [2, 127, 128, 129, 2048])
def test_strided(m):
    a = CASES[f"strided-{m}"].fills[0]
    assert a.size == 5 * TILE + 3 and a.size % 2 == 1
    assert np.array_equal(a, np.arange(a.size) % m)
    own = _owners([a])[0]
    assert own[:m].all() and not own[m:].any()
    for t in range(0, a.size - TILE + 1, TILE):  # every whole tile sees every key
        assert np.unique(a[t:t + TILE]).size == m


@pytest.mark.parametrize("r", [64, 128, 513])
def test_runs(r):
    a = CASES[f"runs-{r}"].fills[0]
    assert a.size == 5 * TILE + 3
    change = np.flatnonzero(a[1:] != a[:-1]) + 1
    assert np.array_equal(change, np.arange(r, a.size, r))   # a new key exactly every r items
    assert np.unique(a).size == change.size + 1              # and never an old one again
    own = _owners([a])[0]
    assert np.array_equal(np.flatnonzero(own), np.arange(0, a.size, r))


def test_descending():
    c = CASES["descending"]
    a, b = c.fills
    n = a.size
    assert np.array_equal(a, np.arange(n)[::-1]) and np.array_equal(b, np.arange(n))
    want = D.expected("descending")
    assert np.array_equal(want[1].local, np.arange(n)[::-1]) and want[1].num_items == n


def test_colliding():
    c = CASES["colliding-64"]
    keys = c.marks["keys"]
    assert c.num_node is None and keys.size == 64 == np.unique(keys).size
    assert (keys & 63 == 0).all()                      # all probe from bucket 0 of a 64-bucket table
    assert 0 in keys and (keys >> 31).any() and 0xFFFFFFFF not in keys
    for f in c.fills:
        assert set(f.tolist()) == set(keys.tolist())   # 64 distinct keys: the table is at 100 %
    assert c.fills[0].size == 3 * 64                   # with repeated instances
    # triangular steps over 64 buckets visit every bucket once in 64 steps (the bound find / find_or_claim rely on)
    pos, seen = 0, []
    for delta in range(1, 65):
        seen.append(pos)
        pos = (pos + delta) & 63
    assert sorted(seen) == list(range(64))


@pytest.mark.parametrize("name", list(CASES))
def test_alignment_and_universe_claims(name):
    c = CASES[name]
    for f in c.fills:
        assert f.dtype == np.uint32 and f.flags.c_contiguous and f.size > 0
        assert int(f.max()) != 0xFFFFFFFF
        if c.num_node is not None:
            assert int(f.max()) < c.num_node
    assert c.capacity >= D.expected(name)[-1].num_items
    # the misaligned runs pass np.concatenate([[0], f])[1:]: 4 bytes off a 16-byte boundary whatever the base
    t = np.concatenate([np.zeros(1, np.uint32), c.fills[0]])
    assert (t[1:].ctypes.data - t.ctypes.data) == 4


@pytest.mark.parametrize("name", list(CASES))
def test_references_agree(name):
    """numpy reference == dict-loop restatement == oracle.HashTable (where the keys fit its direct universe)."""
    c = CASES[name]
    want, again = D.expected(name), D.reference_py(c.fills)
    orc = None
    if c.num_node is not None:
        orc = oracle.HashTable(c.num_node, c.capacity)
        orc.reset()
    for f, w, a in zip(c.fills, want, again):
        assert np.array_equal(w.unique, a.unique) and np.array_equal(w.local, a.local)
        assert np.unique(w.unique).size == w.unique.size
        assert np.array_equal(w.unique[w.local], f)  # the id of every instance leads back to its key
        if orc is not None:
            assert orc.fill_with_duplicates(f) == w.num_items
            assert np.array_equal(orc.unique(), w.unique)
            loc, _ = orc.map_edges(f, f)
            assert np.array_equal(loc, w.local)


def _ok(want, unique, local):
    D.compare_fill(want, unique.size, unique, local, np.arange(unique.size, dtype=np.uint32))


def _last_occurrence_owns(fills):
    """what a dedup that lets the LAST instance of a key own it would give (per fill; the prefix is kept)"""
    uniq, out = [], []
    for a in fills:
        have = set(uniq)
        new = [k for k in dict.fromkeys(a[::-1].tolist()) if k not in have][::-1]  # new keys in last-occurrence order
        uniq = uniq + new
        pos = {k: i for i, k in enumerate(uniq)}
        out.append((np.array(uniq, np.uint32), np.array([pos[k] for k in a.tolist()], np.uint32)))
    return out


@pytest.mark.parametrize("name", ["boundary_pairs", "boundary_pairs-chunks4", "mirrored", "strided-129", "strided-2"])
def test_comparator_rejects_wrong_outputs(name):
    c = CASES[name]
    want = D.expected(name)
    for w in want:  # the right output passes
        _ok(w, w.unique, w.local)
    # 1. last occurrence owns: the same key set, another order
    wrong = _last_occurrence_owns(c.fills)
    differs = False
    for w, (u, l) in zip(want, wrong):
        assert set(u.tolist()) == set(w.unique.tolist())
        if not np.array_equal(u, w.unique):
            differs = True
            with pytest.raises(AssertionError):
                _ok(w, u, l)
    assert differs, "the pattern cannot tell first from last occurrence"
    # 2. ids not contiguous: one id skipped (the count says one more than there are keys) / one id used twice
    w = want[0]
    gap = np.where(w.local >= w.num_items // 2, w.local + 1, w.local).astype(np.uint32)
    with pytest.raises(AssertionError):
        _ok(w, w.unique, gap)
    with pytest.raises(AssertionError):
        D.compare_fill(w, w.num_items + 1, w.unique, w.local, np.arange(w.num_items, dtype=np.uint32))
    twice = np.where(w.local == w.num_items - 1, 0, w.local).astype(np.uint32)
    if w.num_items > 1:
        with pytest.raises(AssertionError):
            _ok(w, w.unique, twice)
        perm = np.arange(w.num_items, dtype=np.uint32)
        perm[[0, w.num_items - 1]] = perm[[w.num_items - 1, 0]]
        with pytest.raises(AssertionError):  # the table's own look-up of its unique list is not the identity
            D.compare_fill(w, w.num_items, w.unique, w.local, perm)
    # 3. prefix not kept: a later fill's list holds the right keys but the earlier fill's part is reordered
    if len(want) > 1 and want[0].num_items > 1:
        w1 = want[1]
        u = w1.unique.copy()
        u[[0, want[0].num_items - 1]] = u[[want[0].num_items - 1, 0]]
        pos = {k: i for i, k in enumerate(u.tolist())}
        l = np.array([pos[k] for k in c.fills[1].tolist()], np.uint32)
        assert set(u.tolist()) == set(w1.unique.tolist()) and np.array_equal(u[l], c.fills[1])  # self-consistent, yet wrong
        with pytest.raises(AssertionError):
            _ok(w1, u, l)
