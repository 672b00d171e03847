"""Shared by the Q8ROW table tests: the numpy reference of the decode (include/ggms.h: float32(float32(code * scale) +
bias), then feat_convert_common.from_f32), a table in which a wrong row's scale or bias cannot pass, and a dataset writer."""
import numpy as np

from feat_convert_common import BF16, BITS, F16, F32, from_f32

Q8ROW = 18  # ggms_dtype code (include/ggms.h)
OUTS = (F32, F16, BF16)
OUT_IDS = ["F32", "F16", "BF16"]
SPECIAL_ROWS = 259  # a table of more rows than this carries the rounding-edge rows 256 .. 258 (make_table)


def stride(dim):
    """Bytes from one stored row to the next: codes, pad to a multiple of 8, float32 scale, float32 bias."""
    return (dim + 7) // 8 * 8 + 8


def decode_f32(codes, scale, bias):
    """The yardstick: an IEEE single multiply, then an IEEE single add (numpy keeps the two apart)."""
    prod = codes.astype(np.float32) * scale.astype(np.float32)[:, None]
    return prod + bias.astype(np.float32)[:, None]


class Table:
    """Packed rows (pad bytes 0xFF: they must never be decoded) and, computed once and read-only, the expected bits of
    every row in each output dtype."""

    def __init__(self, codes, scale, bias):
        from xgnn_amd import datagen
        self.codes, self.scale, self.bias = codes, scale.astype(np.float32), bias.astype(np.float32)
        self.dim = codes.shape[1]
        self.rows = datagen.pack_q8row(codes, self.scale, self.bias)
        self.rows[:, self.dim:stride(self.dim) - 8] = 0xFF
        value = decode_f32(codes, self.scale, self.bias)
        # nothing here may depend on subnormal handling (left unspecified): zero, or at least 2^-100
        for a in (value, self.scale):
            assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= 2.0 ** -100)).all()
        self.bits = {dt: from_f32(np.ascontiguousarray(value), dt) for dt in OUTS}
        for a in (self.rows, *self.bits.values()):
            a.setflags(write=False)

    def want(self, out_dt, index):
        return self.bits[out_dt][index]


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
    return Table(codes, scale, bias)


def write_q8row_dataset(path, dim, num_node=3000, num_train=500, seed=5):
    """feat_convert_common.write_feat_dataset's graph, labels and train set with the Q8ROW table of make_table."""
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(num_node, mean_deg=15, seed=seed)
    train = np.random.RandomState(seed).permutation(num_node)[:num_train].astype(np.uint32)
    table = make_table(num_node, dim, seed + Q8ROW)
    label = (np.arange(num_node, dtype=np.int64) * 7) % 13
    g = dict(indptr=ip, indices=ix, train_set=train, meta=dict(feat_dim=dim, num_class=13))
    datagen.write_dataset(str(path), g, feat=table.rows, label=label, feat_dtype="Q8ROW")
    return dict(ip=ip, ix=ix, train=train, table=table, label=label, path=str(path), dim=dim)


__all__ = ["BF16", "BITS", "F16", "F32", "Q8ROW", "OUTS", "OUT_IDS"]
