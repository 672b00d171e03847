"""Shared by the FP8 table tests: the 256-entry truth tables of the two OCP formats (from torch's CPU cast and from a
closed form that never touches torch's FP8 types), the expected output bits of a decoding gather, and a dataset writer."""
import numpy as np
import torch

from feat_convert_common import BF16, BITS, F16, F32, from_f32, to_f32

E4M3, E5M2 = 16, 17  # ggms_dtype codes (include/ggms.h)
FP8 = (E4M3, E5M2)
OUTS = (F32, F16, BF16)
FP8_NAMES = {E4M3: "F8E4M3", E5M2: "F8E5M2"}
FP8_TORCH = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
FP8_PAIRS = [(s, d) for s in FP8 for d in OUTS]


def truth_torch(fmt):
    """f32 value of every code, by torch's CPU cast."""
    return torch.arange(256, dtype=torch.uint8).view(FP8_TORCH[fmt]).to(torch.float32).numpy()


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


def assert_decoded(got_bits, table_bytes, fmt, out_dt, what=""):
    """Bitwise equal to the truth wherever the code is not NaN (so -0.0 stays -0.0 and inf stays inf); NaN where it is."""
    want = decode_bits(table_bytes, fmt, out_dt)
    assert got_bits.shape == want.shape, (what, got_bits.shape, want.shape)
    want_nan = np.isnan(truth(fmt)[table_bytes])
    got_nan = np.isnan(to_f32(got_bits, out_dt))
    assert np.array_equal(got_nan, want_nan), f"{what}: NaN positions differ"
    bad = (got_bits != want) & ~want_nan
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at flat index {i}: code "
                             f"{int(table_bytes.ravel()[i]):#x} -> got {int(got_bits.ravel()[i]):#x}, want "
                             f"{int(want.ravel()[i]):#x}")


def table_bytes(shape, seed):
    """Bytes of an FP8 table: the first 256 elements of column 0 enumerate every code (where the table has that many
    rows), everything else is random bytes -- so every code also turns up at every position of a chunk."""
    rows, dim = shape
    b = np.random.RandomState(seed).randint(0, 256, (rows, dim)).astype(np.uint8)
    k = min(rows, 256)
    b[:k, 0] = np.arange(k, dtype=np.uint8)
    return b


def write_fp8_dataset(path, fmt, dim, num_node=3000, num_train=500, seed=5):
    """feat_convert_common.write_feat_dataset's graph, labels and train set with an FP8 table of table_bytes."""
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(num_node, mean_deg=15, seed=seed)
    train = np.random.RandomState(seed).permutation(num_node)[:num_train].astype(np.uint32)
    feat = table_bytes((num_node, dim), seed + fmt)
    label = (np.arange(num_node, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=dim, num_class=13))
    datagen.write_dataset(str(path), g, feat=torch.from_numpy(feat).view(FP8_TORCH[fmt]), label=label,
                          feat_dtype=FP8_NAMES[fmt])
    return dict(ip=ip, ix=ix, train=train, feat=feat, label=label, path=str(path), dtype=fmt)


__all__ = ["BF16", "BITS", "F16", "F32", "E4M3", "E5M2", "FP8", "OUTS", "FP8_NAMES", "FP8_TORCH", "FP8_PAIRS"]
