"""GGMS_MXFP4 as the tests state it (not a test): the 16-entry closed form of E2M1, the decode of unpacked rows, and the
feat_formats.Family whose tables put every (code, scale byte) pair into the index head.  Importing it registers the
dtype code with feat_formats' dictionaries (uint8 rows, as for Q8ROW), which tests/gather_harness.py looks formats up in."""
import numpy as np
import torch

import feat_formats as ff

MXFP4 = 20
SCALES = (2, 126, 127, 128, 252, 255)  # both ends of what the encoder writes, around 1.0, and NaN
MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
HEAD = 16 * len(SCALES)
ff.NAMES[MXFP4], ff.BITS[MXFP4], ff.TORCH[MXFP4], ff.TORCH_BITS[MXFP4] = "MXFP4", np.uint8, torch.uint8, torch.uint8


def stride(dim):
    return (17 * ((dim + 31) // 32) + 7) // 8 * 8


def decode(codes, scale_bytes):
    """float32 values of (n, dim) codes under (n, ceil(dim / 32)) scale bytes: sign x magnitude x 2^(x - 127), computed in
    float64 (exact, and a normal f32 or 0 for x in 2 .. 252); NaN where x is 255."""
    x = np.repeat(scale_bytes.astype(np.float64), 32, axis=1)[:, :codes.shape[1]]
    value = np.where(codes & 8, -1.0, 1.0) * MAGNITUDES[codes & 7] * 2.0 ** (x - 127.0)
    with np.errstate(over="ignore"):  # (bytes 253 and 254 may overflow: unspecified, and in no table here)
        return np.where(x == 255, np.nan, value).astype(np.float32)


def table(codes, scale_bytes):
    """The Table of packed rows; the pad bytes behind the scale bytes hold 0xFF: they must never be decoded."""
    from xgnn_amd import datagen
    rows = datagen.pack_mxfp4(codes, scale_bytes)
    rows[:, 17 * scale_bytes.shape[1]:] = 0xFF
    return ff.Table(MXFP4, rows, decode(codes, scale_bytes), codes)


def make_table(rows, dim, seed):
    """Random codes under scale bytes drawn from SCALES and from 2 .. 252; row r < HEAD holds code r % 16 in element 0,
    its complement in element 1 (the high nibble) and SCALES[r // 16] on its first block."""
    rs = np.random.RandomState(seed)
    codes = rs.randint(0, 16, (rows, dim)).astype(np.uint8)
    nb = (dim + 31) // 32
    scales = np.where(rs.rand(rows, nb) < 0.3, rs.choice(SCALES, (rows, nb)), rs.randint(2, 253, (rows, nb))).astype(np.uint8)
    k = min(rows, HEAD)
    codes[:k, 0], codes[:k, 1] = np.arange(k) % 16, 15 - np.arange(k) % 16
    scales[:k, 0] = np.array(SCALES)[np.arange(k) // 16]
    return table(codes, scales)


# dims: chunks of 2 (2, 34), 4 (100; the widest into f32) and 8 elements (32, 128, 768; into f16 / bf16), one block and
# several, a partial last block (34, 100), rows of fewer than 8 chunks and of more; 65536 is 8192 chunks of 8 elements:
# the one-workgroup-per-row kernel
MX = ff.Family(
    "mxfp4", (MXFP4,), lambda fmt, rows, dim, seed: make_table(rows, dim, seed),
    rows=512, seed=lambda fmt, dim: 2000 + dim, head=HEAD, tail=lambda n: n // 8 if n > 300 else int(n > 1),
    dims=[2, 32, 34, 100, 128, 768],
    calls=[(1, False, False, ff.ALL_ONES), (64, False, False, ff.ALL_ONES), (65, True, False, ff.ALL_ONES),
           (257, False, True, ff.ALL_ONES), (257, True, True, ff.ALL_ONES)],
    long_dims=[65536], long_n=3, long_calls=[(False, False), (True, True)],
    stores=dict(cached=(512, lambda fmt: 21), full=(512, lambda fmt: 21), tiered=(512, lambda fmt: 21)))
