"""Named input patterns for the ordered dedup table, and an independent reference for what it must give.

Uniformly random ids never produce the inputs the dedup protocol's comments argue about (hashtable.hip, DedupInsert in
ggms_device.h): one key n times, chunks made only of owners or of none, duplicates that straddle a segment / round /
tile / chunk boundary.  Every pattern here is a function returning a Case: the fills of ONE table version (uint32
arrays) and the universe they need.  The reference is plain numpy: it uses neither the oracle nor the library.

Constants of the owner scan (hashtable.hip): a thread-block tile is kOwnTile = 2048 items = 4 rounds of 512 items; a
(round, wave) segment is 128 items; a chunk is at most kChunkMaxTiles = 31 tiles, because its owner count travels in 16
bits -- so the fullest chunk holds FULL = 63488 items."""
import functools

import numpy as np

TILE, SEGMENT, ROUND = 2048, 128, 512
CHUNK_MAX_TILES = 31
FULL = CHUNK_MAX_TILES * TILE
assert FULL == 63488 and FULL < 65536

OWNER_SCAN_CHUNKS, OWNER_SCAN_TILES = 1, 2  # GGMS_DEBUG_* knobs (include/ggms.h)


class Case:
    """fills: uint32 arrays entered one after the other into one table version; num_node: the direct layout's universe
    (every key < num_node; None = the keys only fit the hashed layout); chunks: the GGMS_DEBUG_OWNER_SCAN_CHUNKS value
    the pattern is built for (None = default grid); marks: indices / sizes the host tests assert the pattern's property on."""

    def __init__(self, name, fills, num_node, chunks=None, **marks):
        self.name = name
        self.fills = [np.ascontiguousarray(f, dtype=np.uint32) for f in fills]
        self.num_node = num_node
        self.chunks = chunks
        self.marks = marks
        assert all(int(f.max()) != 0xFFFFFFFF for f in self.fills if f.size)  # GGMS_EMPTY_KEY is not a key
        if num_node is not None:
            assert all(int(f.max()) < num_node for f in self.fills if f.size)

    @property
    def capacity(self):  # n2o entries that hold every unique key whatever the pattern
        return sum(f.size for f in self.fills)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------ the reference
class Expect:
    """What the table must hold after one fill: the unique list so far (first-occurrence order, cumulative over the
    fills of the version) and the local id of every instance of THIS fill = its key's position in that list."""

    def __init__(self, unique, local):
        self.unique, self.local = unique, local

    @property
    def num_items(self):
        return self.unique.size


def reference(fills):
    """-> [Expect per fill].  numpy only: the first index of every key in (unique so far ++ fill) orders the list."""
    uniq = np.zeros(0, np.uint32)
    out = []
    for a in fills:
        a = np.asarray(a, np.uint32)
        cat = np.concatenate([uniq, a])
        keys, first = np.unique(cat, return_index=True)  # sorted keys, index of each key's first occurrence
        uniq = cat[np.sort(first)]
        rank = np.empty(keys.size, np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(keys.size)
        out.append(Expect(uniq.copy(), rank[np.searchsorted(keys, a)].astype(np.uint32)))
    return out


def reference_py(fills):
    """The same statement once more as a plain loop over a dict (the host tests hold the two against each other)."""
    pos, out = {}, []
    for a in fills:
        local = np.empty(len(a), np.uint32)
        for i, k in enumerate(np.asarray(a).tolist()):
            local[i] = pos.setdefault(k, len(pos))
        out.append(Expect(np.fromiter(pos.keys(), np.uint32, len(pos)), local))
    return out


@functools.lru_cache(maxsize=None)
def expected(case_name):
    """reference(CASES[case_name].fills), computed once and shared by every test (treat it as read-only)."""
    want = reference(CASES[case_name].fills)
    for e in want:
        e.unique.setflags(write=False)
        e.local.setflags(write=False)
    return want


def compare_fill(want, num_items, unique, local, self_map, what=""):
    """The comparator of every dedup test: the table's state after a fill against an Expect.  unique = the table's
    unique list, local = the look-up of every instance of the fill, self_map = the look-up of the unique list itself.
    Raises AssertionError on the first difference."""
    assert int(num_items) == want.num_items, f"{what}: num_items {num_items} != {want.num_items}"
    np.testing.assert_array_equal(np.asarray(unique, np.uint32), want.unique, err_msg=f"{what}: unique list")
    np.testing.assert_array_equal(np.asarray(local, np.uint32), want.local, err_msg=f"{what}: local ids of the fill")
    np.testing.assert_array_equal(np.asarray(self_map, np.uint32), np.arange(want.num_items, dtype=np.uint32),
                                  err_msg=f"{what}: map(unique) != arange")


# ------------------------------------------------------------------ the patterns
def _perm(n, seed):
    return np.random.RandomState(seed).permutation(n).astype(np.uint32)


def all_same(n):
    """One key n times: every instance but index 0 loses, and every candidate on the way down is beaten exactly once
    (the `lost` argument of DedupInsert).  Fill 2: the same again -- no owner at all; fill 3: n copies of another key."""
    return Case(f"all_same-{n}", [np.full(n, 7, np.uint32), np.full(n, 7, np.uint32), np.full(n, 3, np.uint32)], 16)


def all_distinct_full_chunks(k, extra=0):
    """k full chunks (with GGMS_DEBUG_OWNER_SCAN_CHUNKS = k): fill 1 a random permutation -- every item owns, every
    chunk's descriptor carries 63488; fill 2 the same array -- every chunk carries 0; fill 3 the array reversed with
    fresh ids in the last tile only.  extra = 1: one item more than k chunks can take (chunk_fits is false): the
    tile-chained kernel must give the same."""
    n = k * FULL + extra
    a = _perm(n, 100 + k)
    c = a[::-1].copy()
    c[n - TILE:] = n + _perm(TILE, 200 + k)
    return Case(f"all_distinct_full_chunks-{k}" + ("-plus1" if extra else ""), [a, a.copy(), c], n + TILE, chunks=k, k=k,
                extra=extra)


def all_distinct_register_chunks():
    """The same three fills at the other form's edge: 3 chunks of two tiles each (OWNER_SCAN_CHUNKS = 3) stay in
    registers, and a chunk of owners only parks 4096 keys in LDS -- all the workgroup's key buffer holds."""
    n = 3 * 2 * TILE
    a = _perm(n, 300)
    c = a[::-1].copy()
    c[n - TILE:] = n + _perm(TILE, 301)
    return Case("all_distinct_register_chunks", [a, a.copy(), c], n + TILE, chunks=3)


def boundary_pairs(chunks=None):
    """Distinct ids but: one key at {b - 1, b} for every boundary b (segment 128, round 512, tile 2048 and 2 * 2048, the
    first item of chunk 1 and of the last chunk), one key at 0 and n - 1.  n is odd.
    chunks None: the default grid, one tile per chunk; 3: two tiles per chunk (held in registers); 4: three tiles per
    chunk (re-read form)."""
    n = {None: 9 * TILE + 1001, 3: 5 * TILE + 1001, 4: 9 * TILE + 1001}[chunks]
    tiles = (n + TILE - 1) // TILE
    grid = min(tiles, chunks or 1024)
    per = (tiles + grid - 1) // grid
    nchunks = (tiles + per - 1) // per
    bounds = sorted({SEGMENT, ROUND, TILE, 2 * TILE, per * TILE, (nchunks - 1) * per * TILE})
    a = _perm(n, 7)
    for b in bounds:
        a[b] = a[b - 1]
    a[n - 1] = a[0]
    return Case("boundary_pairs" + (f"-chunks{chunks}" if chunks else ""), [a, _perm(n, 8)], n, chunks=chunks, bounds=bounds,
                per=per, nchunks=nchunks)


def mirrored():
    """a[i] == a[n - 1 - i]: every key twice, all owners in the first half."""
    half = _perm(3 * TILE + 77, 9)
    return Case("mirrored", [np.concatenate([half, half[::-1]])], half.size)


def strided(m):
    """a[i] = i % m: every segment / tile sees every key, the owners are the first m items."""
    n = 5 * TILE + 3
    return Case(f"strided-{m}", [(np.arange(n) % m).astype(np.uint32)], max(m, 4), m=m)


def runs(r):
    """Each key r times in a row: a whole wave (64) or segment (128) is one key; 513 straddles every round."""
    n = 5 * TILE + 3
    nkeys = (n + r - 1) // r
    return Case(f"runs-{r}", [_perm(nkeys, 11)[np.arange(n) // r]], max(nkeys, 4), r=r)


def descending():
    """ids n - 1 .. 0, then the same ascending: fill 2 has no owner and maps to the reversed positions."""
    n = 5 * TILE + 3
    a = np.arange(n, dtype=np.uint32)
    return Case("descending", [a[::-1].copy(), a], n)


def colliding(buckets, dups=True):
    """Hashed layout only: `buckets` keys that are all multiples of `buckets`, so all probe from bucket 0 of a table of
    that many buckets and the last one entered needs every step of the probe sequence.  Key 0 is one of them, and one
    with bit 31 set.  Fill 2: every key again (found, none owns)."""
    keys = np.array([j * buckets for j in range(buckets - 1)] + [0x80000000 + buckets], np.uint64).astype(np.uint32)
    rng = np.random.RandomState(buckets)
    first = keys[rng.permutation(buckets)]
    if dups:  # every key once in a random order, then 2 * buckets random repeats
        first = np.concatenate([first, keys[rng.randint(0, buckets, 2 * buckets)]])
    return Case(f"colliding-{buckets}", [first, keys[::-1].copy()], None, keys=keys)


def _all_cases():
    cs = [all_same(n) for n in (1, 2, 2047, 2048, 2049, 100_000)]
    cs += [all_distinct_full_chunks(k) for k in (1, 2, 3)]
    cs += [all_distinct_full_chunks(k, extra=1) for k in (1, 2, 3)]
    cs += [all_distinct_register_chunks()]
    cs += [boundary_pairs(c) for c in (None, 3, 4)]
    cs += [mirrored()]
    cs += [strided(m) for m in (2, 127, 128, 129, 2048)]
    cs += [runs(r) for r in (64, 128, 513)]
    cs += [descending(), colliding(64)]
    return {c.name: c for c in cs}


CASES = _all_cases()
DIRECT_CASES = [n for n, c in CASES.items() if c.num_node is not None]
