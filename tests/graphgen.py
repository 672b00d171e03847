"""Seeded synthetic CSR graphs / features for the tests (numpy; the torch twins import torch when called)."""
import numpy as np


def powerlaw_csr(num_node, mean_deg=8.0, alpha=0.8, dmax=None, seed=0, zero_frac=0.05):
    """In-neighbour CSR with power-law degrees, uniform random neighbours.

    Some nodes get degree 0 (zero_frac) so the len==0 / len<=fanout branches of
    every sampler are exercised.
    """
    rng = np.random.RandomState(seed)
    u = rng.random_sample(num_node)
    deg = np.floor(u ** (-alpha)).astype(np.int64)
    deg = np.maximum(1, (deg * (mean_deg / max(deg.mean(), 1e-9))).astype(np.int64))
    if dmax is None:
        dmax = max(4, num_node // 2)
    deg = np.minimum(deg, dmax)
    deg[rng.random_sample(num_node) < zero_frac] = 0
    indptr = np.zeros(num_node + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, num_node, size=int(indptr[-1])).astype(np.uint32)
    return indptr, indices


def hub_csr(num_node=3000, num_hub=6, hub_deg=6000, base_deg=9, seed=0):
    """A few very long neighbour lists among short ones: the samplers' per-list limits (khop3 fanout 127, khop0's
    heavy-list path and its LDS slot budget) and tail behaviour."""
    rng = np.random.RandomState(seed)
    deg = np.full(num_node, base_deg, np.int64)
    deg[rng.permutation(num_node)[:num_hub]] = hub_deg
    deg[rng.random_sample(num_node) < 0.03] = 0
    indptr = np.zeros(num_node + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(deg)
    indices = rng.randint(0, num_node, size=int(indptr[-1])).astype(np.uint32)
    return indptr, indices


# ---- the feature code ---------------------------------------------------------------------------------------------------
# feat[i, j] = the top bits of a 64-bit mix of the element number i * dim + j, as many as the dtype holds exactly as an
# integer.  The element number is mixed at its full 64 bits: rows any power of two of bytes (or elements) apart differ,
# so a gather that loses high bits of row * row_bytes delivers a row with OTHER contents.  (The form before this one,
# (i * dim + j) & 0xFFFF, repeated every 65536 / gcd(dim, 65536) rows -- and 2^31 and 2^32 bytes are multiples of every
# such period, test_feature_code.py.)
_MIX_ADD, _MIX_M1, _MIX_M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB  # the splitmix64 finaliser's
_CODE_BITS = {"float32": 24, "float64": 24, "int32": 24, "int64": 24, "float16": 11, "bfloat16": 8, "int16": 15, "uint8": 8}


def code_bits(dtype):
    """How many bits of code an element of `dtype` (numpy or torch) holds exactly as a non-negative integer."""
    name = str(dtype).replace("torch.", "")
    return _CODE_BITS[name if name in _CODE_BITS else np.dtype(dtype).name]


def feature_code(elem, bits):
    """The code of element numbers `elem` (any integer array, taken as uint64): int64 values below 2^bits."""
    with np.errstate(over="ignore"):
        x = np.asarray(elem).astype(np.uint64) + np.uint64(_MIX_ADD)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(_MIX_M1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(_MIX_M2)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(64 - bits)).astype(np.int64)


def feature_rows(node_ids, dim, dtype=np.float32):
    """Rows `node_ids` of the (any number of rows) x dim feature table of `dtype`."""
    ids = np.asarray(node_ids).astype(np.uint64)
    elem = ids[:, None] * np.uint64(dim) + np.arange(dim, dtype=np.uint64)[None, :]
    return feature_code(elem, code_bits(dtype)).astype(dtype)


def exact_features(num_node, dim, dtype=np.float32):
    """The num_node x dim feature table: small non-negative integers, exactly representable in `dtype`, aperiodic."""
    return feature_rows(np.arange(num_node, dtype=np.uint64), dim, dtype)


def _signed64(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def _lsr(x, k):
    """Logical right shift of an int64 tensor: the arithmetic one, then a mask over the copies of the sign."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def torch_feature_code(elem, bits):
    """feature_code on an int64 torch tensor (any device): the same arithmetic modulo 2^64 in two's complement."""
    x = elem + _signed64(_MIX_ADD)
    x = (x ^ _lsr(x, 30)) * _signed64(_MIX_M1)
    x = (x ^ _lsr(x, 27)) * _signed64(_MIX_M2)
    x = x ^ _lsr(x, 31)
    return _lsr(x, 64 - bits)


def torch_feature_rows(node_ids, dim, dtype, out=None):
    """feature_rows on the device of `node_ids` (an integer torch tensor), 2^26 elements at a time: into `out`
    (node_ids.numel() x dim, any dtype that holds the code) or a new tensor of `dtype`."""
    import torch
    chunk = max(1, (1 << 26) // dim)
    if out is None:
        out = torch.empty((node_ids.numel(), dim), dtype=dtype, device=node_ids.device)
    cols = torch.arange(dim, dtype=torch.int64, device=node_ids.device)
    bits = code_bits(dtype)
    for lo in range(0, node_ids.numel(), chunk):
        ids = node_ids[lo:lo + chunk].to(torch.int64)
        out[lo:lo + chunk] = torch_feature_code(ids[:, None] * dim + cols[None, :], bits).to(out.dtype)
    return out


def torch_fill_features(table, dtype=None, first_row=0):
    """Fills the 2-D device tensor `table` with rows first_row .. of the feature table of `dtype` (default: its own)."""
    import torch
    rows, dim = table.shape
    chunk = max(1, (1 << 26) // dim)
    for lo in range(0, rows, chunk):
        ids = torch.arange(first_row + lo, first_row + min(rows, lo + chunk), dtype=torch.int64, device=table.device)
        torch_feature_rows(ids, dim, dtype or table.dtype, out=table[lo:lo + chunk])
    return table


def prefix_sums(indptr, weights):
    """Per-neighbour-list inclusive prefix sums in float32 (the prob_prefix_table.bin layout)."""
    import numpy as np
    out = np.zeros(weights.size, np.float32)
    for v in range(indptr.size - 1):
        a, b = int(indptr[v]), int(indptr[v + 1])
        if b > a:
            out[a:b] = np.cumsum(weights[a:b], dtype=np.float32)
    return out


# The literal inputs of the reference's own hash-table unit test (samgraph/unittest/test_hashmap.cc:98-126,166-198):
# successive FillWithDuplicates calls on one table.  What that test asserts -- and ours with it -- is set equality
# with the inputs so far, no duplicates in the unique list, and that each fill keeps the previous list as a prefix.
REF_HASHMAP_VECTORS = {
    "DupRevised_Ref": [[1, 2, 3, 4, 5, 2, 5, 1, 10, 233],
                       [1, 2, 3, 6, 9, 2, 8, 1, 3, 7, 1023],
                       [1, 2, 3, 4, 5, 2, 5, 1, 10, 233, 1, 2, 3, 6, 9, 2, 8, 1, 3, 7, 1023]],
    "MixedFillMethod": [[1, 2, 3, 4, 5, 2, 5, 1, 10, 256, 6, 9, 2, 13, 5, 64, 512, 1021],
                        list(range(1, 513))],
}
REF_HASHMAP_EXPECT = {"MixedFillMethod": [13, 513]}  # EXPECT_EQ(h_set.size(), 13) / EXPECT_EQ(output_uniq.size(), 513)


# ---- a small graph at high edge positions ----------------------------------------------------------------------------
class SparseIndices:
    """`indices` of a high-offset CSR for the numpy references: ix[a:b] and ix[e] at the REAL edge positions.  Positions
    below head.size and from tail_start on exist; the filler's list in between does not, and reading it is an error."""

    def __init__(self, head, tail, tail_start):
        self.head, self.tail, self.tail_start = head, tail, int(tail_start)
        self.size, self.dtype = self.tail_start + tail.size, head.dtype

    def __len__(self):
        return self.size

    def __getitem__(self, k):
        if isinstance(k, slice):
            a, b, step = k.indices(self.size)
            assert step == 1
            if a >= b:
                return self.head[:0]
            if b <= self.head.size:
                return self.head[a:b]
            assert a >= self.tail_start, "the filler's list is never read"
            return self.tail[a - self.tail_start:b - self.tail_start]
        k = int(k)
        if k < self.head.size:
            return self.head[k]
        assert self.tail_start <= k < self.size, "the filler's list is never read"
        return self.tail[k - self.tail_start]


class HighOffsetCSR:
    """What high_offset_csr returns (see there)."""


def high_offset_csr(boundary, num_node=3000, hub_deg=6000, seed=0, device="cuda"):
    """A CSR of num_node real nodes -- power-law degrees, some empty lists -- plus one hub of hub_deg neighbours and one
    FILLER node, whose list is never read: its id occurs in no list (and must occur in no seed list), and its length
    is chosen so that edge position `boundary` lies in the middle of the hub's list, which follows it.  The real nodes
    before the filler lie entirely below the boundary, those behind the hub entirely above.

    Attributes of the result:
      indptr           the real offsets (uint32, num_node + 3 entries; E = indptr[-1] is a little above `boundary`)
      filler, hub      the two node ids;  below / above: the real node ids on either side
      indices          the device array: torch.empty(E) int32, the real lists written (and the filler's id in its own)
      head, tail       the real lists' values before / behind the filler;  tail_start = the hub's first position
      indptr_shifted, indices_shifted   the same graph with the filler at degree 0: what the oracle is called with.  No
                       kernel may touch the filler's list, so results on `indices` equal the shifted graph's.
      ix               SparseIndices over head / tail for the numpy references that index by real position
      restore()        writes head / tail into `indices` again (after a sampler that permutes lists in place)"""
    import torch
    rng = np.random.RandomState(seed)
    ip0, _ = powerlaw_csr(num_node, mean_deg=12.0, dmax=300, seed=seed)
    deg0 = np.diff(ip0.astype(np.int64))
    g = HighOffsetCSR()
    g.filler = num_node // 2
    g.hub = g.filler + 1
    deg = np.concatenate([deg0[:g.filler], [0, hub_deg], deg0[g.filler:]])
    total = deg.size  # num_node + 2
    ea = int(deg[:g.filler].sum())
    fill = int(boundary) - hub_deg // 2 - ea
    assert fill > 0
    g.indptr_shifted = np.zeros(total + 1, np.uint32)
    g.indptr_shifted[1:] = np.cumsum(deg)
    deg[g.filler] = fill
    real = np.zeros(total + 1, np.int64)
    real[1:] = np.cumsum(deg)
    assert real[-1] < 1 << 32 and real[g.hub] < boundary < real[g.hub + 1]
    g.indptr = real.astype(np.uint32)
    nb = rng.randint(0, total - 1, int(g.indptr_shifted[-1]))
    nb[nb >= g.filler] += 1  # every id but the filler's
    g.indices_shifted = nb.astype(np.uint32)
    g.head, g.tail, g.tail_start = g.indices_shifted[:ea], g.indices_shifted[ea:], ea + fill
    g.ix = SparseIndices(g.head, g.tail, g.tail_start)
    g.below = np.arange(0, g.filler, dtype=np.uint32)
    g.above = np.arange(g.hub + 1, total, dtype=np.uint32)
    g.boundary, g.num_edge = int(boundary), int(real[-1])
    # (the filler's list holds the filler's own id: a kernel that strays into it reads a valid node id, whose list is
    # the filler's again -- a wrong result, never a wild index)
    g.indices = torch.empty(g.num_edge, dtype=torch.int32, device=device)
    g.indices[ea:g.tail_start] = g.filler

    def restore():
        g.indices[:ea] = torch.from_numpy(g.head.view(np.int32)).to(device)
        g.indices[g.tail_start:] = torch.from_numpy(g.tail.view(np.int32)).to(device)
    g.restore = restore
    restore()
    return g


def high_offset_table(g, values_shifted, device="cuda"):
    """A per-edge table (prob / alias / prefix sums) of a high_offset_csr graph on the device: torch.empty(E) with the
    real part written from `values_shifted` (one value per edge of the shifted graph) and zeros in the filler's."""
    import torch
    v = np.ascontiguousarray(values_shifted)
    v = v.view(np.int32) if v.dtype == np.uint32 else v
    t = torch.empty(g.num_edge, dtype=torch.from_numpy(v[:1]).dtype, device=device)
    t[g.head.size:g.tail_start] = 0
    t[:g.head.size] = torch.from_numpy(v[:g.head.size]).to(device)
    t[g.tail_start:] = torch.from_numpy(v[g.head.size:]).to(device)
    return t
