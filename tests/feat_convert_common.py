"""Shared by the feat_out_dtype tests: tables of raw F16 / BF16 / F32 bits that carry every rounding edge next to random
data, the CPU conversion the gather must reproduce bit for bit, and a dataset writer for such a table."""
import numpy as np
import torch

F32, F16, BF16 = 0, 2, 7  # ggms_dtype codes
NAMES = {F32: "F32", F16: "F16", BF16: "BF16"}
KEYS = {F32: "f32", F16: "f16", BF16: "bf16"}
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
TORCH_BITS = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}
PAIRS = [(F16, F32), (BF16, F32), (F32, F16), (F32, BF16), (F16, BF16), (BF16, F16)]

# +-0, +-inf, NaN; 65504 and 65520 (the f16 overflow tie); 1 + 2^-11, 1 + 3 2^-11 (f16 ties); 1 + 2^-8, 1 + 3 2^-8 (bf16
# ties); 2^-24 and 2^-25 (the f16 subnormal edge); an f32 subnormal; and their negatives
_POS = [0.0, np.inf, 65504.0, 65520.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -24,
        2.0 ** -25, 1e-40, 3 * 2.0 ** -25, 65519.996, 3.4028235e38]
SPECIAL_F32 = np.array(_POS + [-v for v in _POS] + [np.nan], np.float32)
# subnormal inputs of the widening direction (f16: below 2^-14, bf16: below 2^-126), smallest, largest and signed
SPECIAL_BITS16 = np.array([0x0001, 0x03ff, 0x8001, 0x83ff, 0x007f, 0x8040, 0x0200, 0x7c01, 0xfe00], np.uint16)


def to_f32(bits, dt):
    """The exact f32 value of every element of a table of raw bits."""
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


def assert_same_bits(got_bits, want_bits, dt, what=""):
    """Bit-exact wherever the expected value is not NaN; NaN where it is."""
    assert got_bits.shape == want_bits.shape, (what, got_bits.shape, want_bits.shape)
    want_nan = np.isnan(to_f32(want_bits, dt))
    got_nan = np.isnan(to_f32(got_bits, dt))
    assert np.array_equal(got_nan, want_nan), f"{what}: NaN positions differ"
    bad = (got_bits != want_bits) & ~want_nan
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at flat index {i}: "
                             f"got {int(got_bits.ravel()[i]):#x}, want {int(want_bits.ravel()[i]):#x}")


def tensor_bits(t, dt):
    """Raw bits of a torch tensor of dtype TORCH[dt], as a numpy array."""
    return t.contiguous().view(TORCH_BITS[dt]).cpu().numpy().view(BITS[dt])


def write_feat_dataset(path, dt, dim, num_node=3000, num_train=500, seed=5):
    """test_engine.make_dataset's graph (3000 nodes, 500 train nodes) with a `dt` feature table of table_bits."""
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(num_node, mean_deg=15, seed=seed)
    train = np.random.RandomState(seed).permutation(num_node)[:num_train].astype(np.uint32)
    feat = table_bits(dt, (num_node, dim), seed + dt)
    label = (np.arange(num_node, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=dim, num_class=13))
    datagen.write_dataset(str(path), g, feat=feat, label=label, feat_dtype=NAMES[dt])
    return dict(ip=ip, ix=ix, train=train, feat=feat, label=label, path=str(path), dtype=dt)
