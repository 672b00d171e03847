"""The feature-table formats as the tests state them, independently of the library (nothing here reads a header or
imports from xgnn_amd/csrc): dtype codes and names, the CPU conversions the gathers must reproduce bit for bit, the FP8
truth tables, the Q8ROW decode, the quantiser's CPU yardsticks, and one FAMILY object per kind of source -- float (F16 /
BF16 / F32), FP8 (E4M3 / E5M2) and Q8ROW -- that makes host tables, says what a gather of them must deliver, and carries
the parameter lists of its gather tests.  Host code only: importing this module touches no GPU."""
import itertools
import os

import numpy as np
import torch

F32, F16, U8, BF16, E4M3, E5M2, Q8ROW = 0, 2, 3, 7, 16, 17, 18  # ggms_dtype codes (include/ggms.h)
OUTS = (F32, F16, BF16)  # what a converting gather can deliver
ALL_ONES = 0xFFFFFFFF
NAMES = {F32: "F32", F16: "F16", BF16: "BF16", E4M3: "F8E4M3", E5M2: "F8E5M2", Q8ROW: "Q8ROW"}
CODES = {name: code for code, name in NAMES.items()}
KEYS = {F32: "f32", F16: "f16", BF16: "bf16"}  # values of the config key feat_out_dtype
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, E4M3: np.uint8, E5M2: np.uint8, Q8ROW: np.uint8}
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16, E4M3: torch.float8_e4m3fn,
         E5M2: torch.float8_e5m2, Q8ROW: torch.uint8}  # (a Q8ROW table is handed around as uint8 rows)
TORCH_BITS = {F32: torch.int32, F16: torch.int16, BF16: torch.int16, E4M3: torch.uint8, E5M2: torch.uint8,
              Q8ROW: torch.uint8}
TORCH_NAME = {dt: str(t) for dt, t in TORCH.items() if dt != Q8ROW}

# +-0, +-inf, NaN; 65504 and 65520 (the f16 overflow tie); 1 + 2^-11, 1 + 3 2^-11 (f16 ties); 1 + 2^-8, 1 + 3 2^-8 (bf16
# ties); 2^-24 and 2^-25 (the f16 subnormal edge); an f32 subnormal; and their negatives
_POS = [0.0, np.inf, 65504.0, 65520.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -24,
        2.0 ** -25, 1e-40, 3 * 2.0 ** -25, 65519.996, 3.4028235e38]
SPECIAL_F32 = np.array(_POS + [-v for v in _POS] + [np.nan], np.float32)
# subnormal inputs of the widening direction (f16: below 2^-14, bf16: below 2^-126), smallest, largest and signed
SPECIAL_BITS16 = np.array([0x0001, 0x03ff, 0x8001, 0x83ff, 0x007f, 0x8040, 0x0200, 0x7c01, 0xfe00], np.uint16)
SPECIAL_ROWS = 259  # a Q8ROW table of more rows than this carries the rounding-edge rows 256 .. 258 (make_table)


# ---- conversions and comparisons -------------------------------------------------------------------------------------
def to_f32(bits, dt):
    """The exact f32 value of every element of a table of raw F32 / F16 / BF16 bits."""
    if dt == F32:
        return bits.view(np.float32)
    if dt == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def from_f32(vals, dt):
    """Raw bits of f32 values rounded to `dt` (numpy / torch on the CPU: nearest even, subnormals kept)."""
    if dt == F32:
        return vals.view(np.uint32)
    if dt == F16:
        with np.errstate(over="ignore"):
            return vals.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(vals)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def convert_bits(bits, src, dst):
    return from_f32(np.ascontiguousarray(to_f32(bits, src)), dst)


def tensor_bits(t, dt):
    """Raw bits of a torch tensor of dtype TORCH[dt], as a numpy array."""
    return t.contiguous().view(TORCH_BITS[dt]).cpu().numpy().view(BITS[dt])


def assert_bits(got, want, nan_mask, what="", *, dt, codes=None):
    """The one comparison of delivered bits: bit-exact wherever `nan_mask` is false (so -0.0 stays -0.0 and inf stays
    inf), a NaN of any payload where it is true.  `dt` is the dtype the bits are of; `codes` (optional, got's shape) are
    the stored codes the elements were decoded from, named in the message."""
    assert got.shape == want.shape == nan_mask.shape, (what, got.shape, want.shape, nan_mask.shape)
    bad = np.where(nan_mask, ~np.isnan(to_f32(got, dt)), got != want)
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        code = "" if codes is None else f"code {int(np.asarray(codes).ravel()[i]):#x} -> "
        wanted = "NaN" if nan_mask.ravel()[i] else f"{int(want.ravel()[i]):#x}"
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at flat index {i} (row {i // got.shape[-1]} "
                             f"column {i % got.shape[-1]}): {code}got {int(got.ravel()[i]):#x}, want {wanted}")


def sentinel(dt):
    """What an output buffer holds before a call (no NaN, no value a table decodes to by accident)."""
    return 0x5a5a5a5a if dt == F32 else 0x5a5a


def check_output(flat, dt, lead, shape, dst_rows, want, nan_mask, what="", codes=None):
    """Judges one gather output: `flat` are the bits of the whole sentinel-filled buffer, whose elements lead ..
    lead + rows x dim are the `shape` = (rows, dim) output.  Rows `dst_rows` hold `want` (assert_bits); every other
    element -- the canaries on either side, rows past the count, rows outside dst_index -- still holds the sentinel."""
    n = shape[0] * shape[1]
    assert (flat[:lead] == sentinel(dt)).all() and (flat[lead + n:] == sentinel(dt)).all(), \
        f"{what}: bytes outside the output were written"
    body = flat[lead:lead + n].reshape(shape)
    untouched = np.ones(shape[0], bool)
    untouched[dst_rows] = False
    assert (body[untouched] == sentinel(dt)).all(), f"{what}: rows beyond the count / outside dst_index were written"
    assert_bits(body[dst_rows], want, nan_mask, what, dt=dt, codes=codes)


# ---- FP8: the 256-entry truth tables -----------------------------------------------------------------------------------
def truth_torch(fmt):
    """f32 value of every code, by torch's CPU cast."""
    return torch.arange(256, dtype=torch.uint8).view(TORCH[fmt]).to(torch.float32).numpy()


def truth_closed_form(fmt):
    """f32 value of every code from the formats' definition: sign, exponent (bias 7 / 15), mantissa (3 / 2 bits),
    subnormals at exponent 0; E4M3 (fn): only S.1111.111 is NaN, no infinities; E5M2: exponent 31 is inf / NaN."""
    man_bits, bias = (3, 7) if fmt == E4M3 else (2, 15)
    code = np.arange(256, dtype=np.int64)
    sign = np.where(code & 0x80, -1.0, 1.0)
    exp = (code & 0x7f) >> man_bits
    man = (code & ((1 << man_bits) - 1)).astype(np.float64) / (1 << man_bits)
    val = np.where(exp == 0, man * 2.0 ** (1 - bias), (1.0 + man) * 2.0 ** (exp.astype(np.float64) - bias))
    if fmt == E4M3:
        val = np.where((code & 0x7f) == 0x7f, np.nan, val)
    else:
        val = np.where(exp == 31, np.where(man == 0, np.inf, np.nan), val)
    return (sign * val).astype(np.float32)  # exact: every finite code fits f32 (and f16, bf16)


_TRUTH = {}


def truth(fmt):
    """The closed-form table, built once and never written."""
    if fmt not in _TRUTH:
        t = truth_closed_form(fmt)
        t.setflags(write=False)
        _TRUTH[fmt] = t
    return _TRUTH[fmt]


def decode_bits(table_bytes, fmt, out_dt):
    """Raw bits of truth[table_bytes] cast to out_dt on the CPU (the cast is exact for every finite code)."""
    return from_f32(np.ascontiguousarray(truth(fmt)[table_bytes]), out_dt)


# ---- Q8ROW: the row layout and the decode ------------------------------------------------------------------------------
def stride(dim):
    """Bytes from one stored row to the next: codes, pad to a multiple of 8, float32 scale, float32 bias."""
    return (dim + 7) // 8 * 8 + 8


def decode_f32(codes, scale, bias):
    """The yardstick: an IEEE single multiply, then an IEEE single add (numpy keeps the two apart)."""
    prod = codes.astype(np.float32) * scale.astype(np.float32)[:, None]
    return prod + bias.astype(np.float32)[:, None]


# ---- host tables -------------------------------------------------------------------------------------------------------
class Table:
    """A host table of format `fmt`: `stored` is what lies in memory (rows x dim raw bits or FP8 bytes; rows x stride
    bytes of Q8ROW), `value` the exact f32 value of every element, `codes` (FP8, Q8ROW) the 8-bit code behind it.  All
    read-only; the expected bits per output dtype are computed once."""

    def __init__(self, fmt, stored, value, codes=None):
        self.fmt, self.stored, self.value, self.codes = fmt, stored, value, codes
        self.dim, self.row_bytes = value.shape[1], stored.shape[1] * stored.itemsize
        self._bits, self._nan = {fmt: stored}, np.isnan(value)
        for a in (stored, value, self._nan):
            a.setflags(write=False)

    def bits(self, out_dt):
        """Every row as a gather delivers it in out_dt (out_dt = fmt: the stored rows themselves)."""
        if out_dt not in self._bits:
            self._bits[out_dt] = from_f32(np.array(self.value), out_dt)  # (a copy: value is read-only)
            self._bits[out_dt].setflags(write=False)
        return self._bits[out_dt]

    def want(self, out_dt, index):
        return self.bits(out_dt)[index]

    def nan(self, index):
        """Where NaN is expected (no conversion makes or loses one)."""
        return self._nan[index]

    def code_of(self, index):
        return None if self.codes is None else self.codes[index]


def table_bits(dt, shape, seed):
    """Raw bits of a `dt` table: every third element a special case (cycling through all of them), the rest random --
    f32: magnitudes from 1e-9 to 1e6, which spans the f16 subnormals and its overflow; 16-bit types: random BITS."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if dt == F32:
        vals = (rs.standard_normal(n) * 10.0 ** rs.uniform(-9, 6, n)).astype(np.float32)
        special = SPECIAL_F32
        bits = vals.view(np.uint32).copy()
        sbits = special.view(np.uint32)
    else:
        bits = rs.randint(0, 1 << 16, n).astype(np.uint16)
        sbits = np.concatenate([from_f32(SPECIAL_F32, dt), SPECIAL_BITS16])
    pos = np.arange(0, n, 3)
    bits[pos] = sbits[(pos // 3) % sbits.size]
    return bits.reshape(shape)


def table_bytes(shape, seed):
    """Bytes of an FP8 table: the first 256 elements of column 0 enumerate every code (where the table has that many
    rows), everything else is random bytes -- so every code also turns up at every position of a chunk."""
    rows, dim = shape
    b = np.random.RandomState(seed).randint(0, 256, (rows, dim)).astype(np.uint8)
    k = min(rows, 256)
    b[:k, 0] = np.arange(k, dtype=np.uint8)
    return b


def q8row_table(codes, scale, bias):
    """The Table of packed rows (pad bytes 0xFF: they must never be decoded); also keeps `scale` and `bias`."""
    from xgnn_amd import datagen
    scale, bias, dim = scale.astype(np.float32), bias.astype(np.float32), codes.shape[1]
    rows = datagen.pack_q8row(codes, scale, bias)
    rows[:, dim:stride(dim) - 8] = 0xFF
    value = decode_f32(codes, scale, bias)
    # nothing here may depend on subnormal handling (left unspecified): zero, or at least 2^-100
    for a in (value, scale):
        assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= 2.0 ** -100)).all()
    t = Table(Q8ROW, rows, value, codes)
    t.scale, t.bias = scale, bias
    for out_dt in OUTS:
        t.bits(out_dt)
    return t


def make_table(rows, dim, seed):
    """Random codes with column 0 of the first 256 rows enumerating every code.  Scales are 2^e x a random mantissa with
    e in [-20, 0], and a row's neighbour sits at the other end of that range (rows 2k / 2k + 1: e and -20 - e), so the
    scales of neighbouring rows differ by factors up to 2^20; every fifth scale is negative; the bias changes sign from
    row to row and is of the size of the row's range; every seventh row has scale 0 (row 7: bias 0 too).  Rows 256, 257
    and 258 (tables of more than SPECIAL_ROWS rows) produce the f16 overflow tie 65520 = 255 x 256 + 240 and the f16 /
    bf16 ties 1 + 2^-11, 1 + 3 x 2^-11 and 1 + 2^-8, 1 + 3 x 2^-8 exactly."""
    rs = np.random.RandomState(seed)
    codes = rs.randint(0, 256, (rows, dim)).astype(np.uint8)
    k = min(rows, 256)
    codes[:k, 0] = np.arange(k, dtype=np.uint8)
    e = rs.randint(-20, 1, rows)
    e[1::2] = -20 - e[0:rows - 1:2][: e[1::2].size]
    scale = (np.ldexp(1.0 + rs.rand(rows), e)).astype(np.float32)
    scale[::5] *= -1
    bias = (rs.uniform(0.25, 300.0, rows) * np.abs(scale) * np.where(np.arange(rows) % 2, -1.0, 1.0)).astype(np.float32)
    scale[::7] = 0.0
    if rows > 7:
        bias[7] = 0.0
    if rows > SPECIAL_ROWS:
        scale[256:259] = [256.0, 2.0 ** -11, 2.0 ** -8]
        bias[256:259] = [240.0, 1.0, 1.0]
        codes[256:259, 0] = [255, 1, 1]
        if dim > 1:
            codes[257:259, 1] = 3
    return q8row_table(codes, scale, bias)


# ---- the families --------------------------------------------------------------------------------------------------------
class Family:
    """One kind of source table.  `make(fmt, rows, dim, seed)` is its host Table; `pairs` are the (source, output) dtypes
    its gather tests run.  The remaining attributes are the parameter lists of those tests (tests/gather_harness.py):

    rows, seed      the shared gather tables: `rows` rows, made with seed(fmt, dim)
    head            index entries 0 .. head - 1 come first (the rows that enumerate every code, and the edge rows)
    tail(n)         how many of the last index entries repeat the first ones
    dims, calls     the main test: every dim x every (n, scatter, dev_count, mask)
    long_*          the long-row kernel: dims, n, and (scatter, dev_count) per call, on a table of 8 rows
    shift, shifted  `out` shift elements past its aligned base: (dim, n, scatter, dev_count) per call
    offsets         table bases this many bytes past a 256-byte boundary (the (dim, n, scatter) of `offset_calls`)
    stores          the (rows, seed) of the dim-20 tables behind the cached / full-cache / tiered tests
    host_mask       the tiered call's host_row_mask (0: none)
    """

    def __init__(self, name, formats, make, **lists):
        self.name, self.formats, self.make = name, formats, make
        self.pairs = [(s, d) for s in formats for d in OUTS if s != d]
        self.offsets, self.host_mask = (), 0
        self.__dict__.update(lists)
        self._tables = {}

    def table(self, fmt, rows, dim, seed=None):
        """make()'s table, once per argument list (seed None: the shared gather table's seed)."""
        key = (fmt, rows, dim, self.seed(fmt, dim) if seed is None else seed)
        if key not in self._tables:
            self._tables[key] = self.make(*key)
        return self._tables[key]

    def store(self, fmt, kind):
        rows, seed = self.stores[kind]
        return self.table(fmt, rows, 20, seed(fmt))


def _float_table(fmt, bits):
    return Table(fmt, bits, to_f32(bits, fmt))


def _fp8_table(fmt, b):
    return Table(fmt, b, truth(fmt)[b], b)


def pair_id(pair):
    return f"{NAMES[pair[0]]}-{NAMES[pair[1]]}"


_SPARSE_CALLS = [(n, False, False, ALL_ONES) for n in [0, 1, 63, 64, 65, 257, 4097]] + \
    [c for n in [65, 257] for c in [(n, True, False, ALL_ONES), (n, False, True, ALL_ONES), (n, True, True, 255)]]
_LONG = dict(long_dims=[8191, 8193, 8 * 8191, 8 * 8192], long_n=5, long_calls=[(False, False), (True, True)])
_SHIFTED = dict(shift=1, shifted=[c for dim in (128, 20) for c in [(dim, 257, False, False), (dim, 65, True, True)]])

FLOAT = Family(
    "float", (F16, BF16, F32), lambda fmt, rows, dim, seed: _float_table(fmt, table_bits(fmt, (rows, dim), seed)),
    pairs=[(F16, F32), (BF16, F32), (F32, F16), (F32, BF16), (F16, BF16), (BF16, F16)],
    rows=2048, seed=lambda fmt, dim: fmt * 1000 + dim, head=0, tail=lambda n: n // 4,
    # dim: chunks of 1, 1, 2 and 4 elements, then the widest chunk a pair has (8 between the 16-bit types, else 4); rows
    # of fewer than 8 chunks keep 8 loads in flight per lane (dims 1, 7, 6; 32 between the 16-bit types), the others 16
    dims=[1, 7, 6, 100, 32, 128],
    calls=list(itertools.product([0, 1, 63, 64, 65, 1000], [False, True], [False, True], [ALL_ONES, 15])),
    # dim 65536 = 16384 chunks of 4 elements: the one-workgroup-per-row kernel
    long_dims=[65536], long_n=3, long_calls=[(False, False), (True, False)],
    shift=2, shifted=[(128, 65, False, False)],  # two elements: only 2-element chunks stay aligned on the output side
    stores=dict(cached=(500, lambda fmt: 11), full=(500, lambda fmt: 12), tiered=(512, lambda fmt: 13)), host_mask=255)

FP8 = Family(
    "fp8", (E4M3, E5M2), lambda fmt, rows, dim, seed: _fp8_table(fmt, table_bytes((rows, dim), seed)),
    rows=512, seed=lambda fmt, dim: fmt * 1000 + dim, head=256, tail=lambda n: n // 4,
    # dims: chunks of 1 (1, 3), 2 (6, 130), 4 (4, 20, 100; the widest into f32) and 8 elements (8, 128, 768, 1032; into
    # f16 / bf16), rows of fewer than 8 chunks (8 loads in flight per lane) and of more (16), tiles whose chunk count is
    # no multiple of the 64 lanes x loads in flight, and this feature's real shapes
    dims=[1, 3, 4, 6, 8, 20, 100, 128, 130, 768, 1032], calls=_SPARSE_CALLS, **_LONG, **_SHIFTED,
    # the table's base 1, 2 and 4 bytes past a 16-byte boundary: chunks of 1, 2 and 4 elements are what stays aligned
    offsets=(1, 2, 4), offset_calls=[c for dim in (128, 20) for c in [(dim, 257, False), (dim, 65, True)]],
    stores=dict(cached=(500, lambda fmt: 11 + fmt), full=(500, lambda fmt: 12 + fmt), tiered=(512, lambda fmt: 13 + fmt)))

# index head: column 0 of rows 0 .. 255 enumerates every code, 256 .. 258 are the rounding edges; dims: chunks of 1 (1,
# 3), 2 (6, 130), 4 (4, 20, 100; the widest into f32) and 8 codes (8, 128, 768; into f16 / bf16), pad bytes of every
# length from 0 to 7, rows of fewer than 8 chunks (8 loads in flight per lane) and of more (16)
Q8 = Family(
    "q8row", (Q8ROW,), lambda fmt, rows, dim, seed: make_table(rows, dim, seed),
    rows=512, seed=lambda fmt, dim: 1000 + dim, head=260, tail=lambda n: n // 8 if n > 300 else int(n > 1),
    dims=[1, 3, 4, 6, 8, 20, 100, 128, 130, 768], calls=_SPARSE_CALLS, **_LONG, **_SHIFTED,
    stores=dict(cached=(512, lambda fmt: 11), full=(512, lambda fmt: 11), tiered=(512, lambda fmt: 11)))

FAMILIES = (FLOAT, FP8, Q8)
FAMILY = {fmt: fam for fam in FAMILIES for fmt in fam.formats}


# ---- datasets ------------------------------------------------------------------------------------------------------------
def write_dataset(path, fmt, dim, num_node=3000, num_train=500, seed=5):
    """test_engine.make_dataset's graph (3000 nodes, 500 train nodes), its labels and train set, with a feature table of
    format `fmt`: FAMILY[fmt].make(fmt, num_node, dim, seed + fmt)."""
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(num_node, mean_deg=15, seed=seed)
    train = np.random.RandomState(seed).permutation(num_node)[:num_train].astype(np.uint32)
    table = FAMILY[fmt].make(fmt, num_node, dim, seed + fmt)
    label = (np.arange(num_node, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=dim, num_class=13))
    feat = torch.from_numpy(np.array(table.stored)).view(TORCH[fmt]) if fmt in FP8.formats else table.stored
    datagen.write_dataset(str(path), g, feat=feat, label=label, feat_dtype=NAMES[fmt])
    return dict(ip=ip, ix=ix, train=train, table=table, feat=table.stored, label=label, path=str(path), dtype=fmt, dim=dim)


def write_finite_dataset(path, dt, dim, bad_rows=()):
    """write_dataset's F32 / F16 dataset with every NaN / inf of its table replaced by 0.5 (the rounding-edge values and
    the signed zeros stay) -- a row-scaled table has no code for either; bad_rows: {row: value} puts a non-finite value
    back into column 3 of those rows."""
    d = write_dataset(path, dt, dim)
    v = d["feat"].view({F32: np.float32, F16: np.float16}[dt]).copy()
    v[~np.isfinite(v)] = 0.5
    for row, value in dict(bad_rows).items():
        v[row, 3] = value
    v.tofile(os.path.join(d["path"], "feat.bin"))
    d["values"] = v
    return d


# ---- the quantiser's CPU yardsticks --------------------------------------------------------------------------------------
def cpu_q8row(values, first_row=0):
    from xgnn_amd import datagen
    return datagen.pack_q8row(*datagen.quantize_q8row(values, first_row=first_row))


def cpu_fp8(values, fmt):
    """quantize_features' cast, as bytes (fmt: "F8E4M3" / "F8E5M2")."""
    v = torch.from_numpy(np.array(values)).float()  # (a copy: dataset tables are read-only)
    if fmt == "F8E4M3":
        v = v.clamp(-448.0, 448.0)
    return v.to(TORCH[CODES[fmt]]).view(torch.uint8).numpy()


def assert_fp8_bytes(got, values, fmt, what=""):
    """Bytes equal the torch cast wherever the input is not NaN; a NaN code of the format where it is."""
    want = cpu_fp8(values, fmt)
    nan = np.isnan(np.asarray(values, np.float32))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want) & ~nan
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError(f"{what}: {int(bad.sum())} codes differ, first at flat index {i}: input "
                             f"{np.asarray(values).ravel()[i]!r}, got {int(got.ravel()[i]):#x}, want {int(want.ravel()[i]):#x}")
    g = got[nan] & 0x7f
    assert ((g == 0x7f) if fmt == "F8E4M3" else (g > 0x7c)).all(), f"{what}: a NaN input did not give a NaN code"
