"""The Q8ROW row format on the host (include/ggms.h): the stored row stride, pack / unpack, and the per-row quantiser of
xgnn_amd.datagen.quantize_features checked against float64."""
import os

import numpy as np
import pytest

from feat_formats import Q8ROW, stride


def test_pack_unpack_round_trip():
    from xgnn_amd import datagen
    rs = np.random.RandomState(1)
    for dim in (1, 7, 8, 9, 20, 128, 130):
        codes = rs.randint(0, 256, (37, dim)).astype(np.uint8)
        scale = rs.standard_normal(37).astype(np.float32)
        bias = (rs.standard_normal(37) * 1e3).astype(np.float32)
        rows = datagen.pack_q8row(codes, scale, bias)
        assert rows.dtype == np.uint8 and rows.shape == (37, stride(dim)) == (37, datagen.q8row_stride(dim))
        pad = stride(dim) - 8
        assert (rows[:, dim:pad] == 0).all()  # zero bytes up to the trailer
        assert rows[:, pad:pad + 4].tobytes() == scale.astype("<f4").tobytes()  # little-endian float32, scale first
        assert rows[:, pad + 4:].tobytes() == bias.astype("<f4").tobytes()
        c, s, b = datagen.unpack_q8row(rows, dim)
        assert np.array_equal(c, codes) and s.tobytes() == scale.tobytes() and b.tobytes() == bias.tobytes()


def test_row_bytes_of_every_dtype():
    from xgnn_amd import lib, ops
    h = lib()
    sizes = {0: 4, 1: 8, 2: 2, 3: 1, 4: 4, 5: 1, 6: 8, 7: 2, 16: 1, 17: 1}
    for code, es in sizes.items():
        assert h.ggms_dtype_bytes(code) == es
        for dim in (1, 7, 128):
            assert h.ggms_row_bytes(code, dim) == dim * es, (code, dim)
    want = {1: 16, 7: 16, 8: 16, 9: 24, 128: 136, 130: 144}
    assert {dim: h.ggms_row_bytes(Q8ROW, dim) for dim in want} == want
    assert all(stride(dim) == v for dim, v in want.items())
    assert ops.row_bytes(ops.Q8ROW, 128) == 136 and ops.Q8ROW == Q8ROW
    for unknown in (8, 15, 19, 99, -1):
        assert h.ggms_row_bytes(unknown, 128) == 0 and h.ggms_dtype_bytes(unknown) == 0
    assert h.ggms_dtype_bytes(Q8ROW) == 0  # a row format has no element size: the plain entry points refuse the code


def _values(dtype, dim=24):
    """Random rows with magnitudes from 1e-3 to 1e4, a constant row, a row of one value repeated plus a single outlier,
    and negative-only rows."""
    rs = np.random.RandomState(3)
    mag = 10.0 ** rs.uniform(-3, 4, (40, 1))
    v = rs.standard_normal((40, dim)) * mag
    v[5] = 3.25                       # constant
    v[6] = -0.5                       # one value repeated ...
    v[6, 11] = 812.0                  # ... plus a single outlier
    v[7:12] = -np.abs(v[7:12]) - mag[7:12]  # negative only
    v[12] = 0.0                       # constant zero
    return v.astype(dtype)


@pytest.mark.parametrize("name,dtype", [("F32", np.float32), ("F16", np.float16)])
def test_quantize_features(tmp_path, name, dtype):
    from xgnn_amd import datagen
    v = _values(dtype)
    n, dim = v.shape
    from graphgen import powerlaw_csr
    ip, ix = powerlaw_csr(n, mean_deg=4, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(8, dtype=np.uint32), meta=dict(feat_dim=dim, num_class=3))
    datagen.write_dataset(str(tmp_path / "in"), g, feat=v, label=np.zeros(n, np.int64), feat_dtype=name)
    out = datagen.quantize_features(str(tmp_path / "in"), str(tmp_path / "out"), "Q8ROW")
    meta = dict(line.split() for line in open(os.path.join(out, "meta.txt")))
    assert meta["FEAT_DATA_TYPE"] == "Q8ROW" and int(meta["FEAT_DIM"]) == dim
    assert os.path.getsize(os.path.join(out, "feat.bin")) == n * stride(dim)
    assert open(os.path.join(out, "indptr.bin"), "rb").read() == open(os.path.join(str(tmp_path / "in"), "indptr.bin"), "rb").read()
    rows = np.fromfile(os.path.join(out, "feat.bin"), np.uint8).reshape(n, stride(dim))
    assert (rows[:, dim:stride(dim) - 8] == 0).all()
    codes, scale, bias = datagen.unpack_q8row(rows, dim)
    x = v.astype(np.float64)
    lo, hi = x.min(axis=1), x.max(axis=1)
    assert np.array_equal(bias.astype(np.float64), lo)                         # bias = min
    assert np.array_equal(scale, ((hi - lo) / 255.0).astype(np.float32))      # scale = float32((max - min) / 255)
    s = scale.astype(np.float64)[:, None]
    err = np.abs(x - (s * codes.astype(np.float64) + lo[:, None]))
    bound = 0.5 * s + 2.0 ** -22 * (hi - lo)[:, None]
    assert (err <= bound).all(), float((err - bound).max())
    constant = hi == lo
    assert constant[[5, 12]].all() and constant.sum() == 2
    for r in range(n):
        if constant[r]:  # scale 0, codes 0: decodes exactly
            assert scale[r] == 0 and (codes[r] == 0).all() and np.array_equal(np.full(dim, bias[r], np.float64), x[r])
        else:
            assert (codes[r] == 0).any() and (codes[r] == 255).any(), r


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_quantize_features_refuses_a_row_it_cannot_code(tmp_path, bad):
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    v = _values(np.float32)
    v[17, 3] = bad
    n, dim = v.shape
    ip, ix = powerlaw_csr(n, mean_deg=4, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(8, dtype=np.uint32), meta=dict(feat_dim=dim, num_class=3))
    datagen.write_dataset(str(tmp_path / "in"), g, feat=v, label=np.zeros(n, np.int64))
    with pytest.raises(ValueError, match="row 17"):
        datagen.quantize_features(str(tmp_path / "in"), str(tmp_path / "out"), "Q8ROW")
