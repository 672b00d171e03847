"""The two OCP FP8 formats on the host: the truth table every FP8 gather test decodes against (built twice, independently),
the dtype codes, and datagen.quantize_features (no GPU touched)."""
import os

import numpy as np
import pytest
import torch

from feat_formats import BF16, E4M3, E5M2, F16, F32, NAMES, TORCH, decode_bits, to_f32, truth, truth_closed_form, truth_torch

FP8 = (E4M3, E5M2)


@pytest.mark.parametrize("fmt", FP8, ids=[NAMES[f] for f in FP8])
def test_truth_table_torch_and_closed_form_agree(fmt):
    a, b = truth_torch(fmt), truth_closed_form(fmt)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    assert np.array_equal(nan_a, nan_b)
    assert np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])  # bitwise: -0.0 is 0x80, not 0x00
    nan_codes, inf_codes = np.flatnonzero(nan_b).tolist(), np.flatnonzero(np.isinf(b)).tolist()
    if fmt == E4M3:
        assert nan_codes == [0x7f, 0xff] and inf_codes == []
        assert b[0x7e] == 448.0 and b[0xfe] == -448.0 and b[0x01] == 2.0 ** -9
    else:
        assert nan_codes == [0x7d, 0x7e, 0x7f, 0xfd, 0xfe, 0xff] and inf_codes == [0x7c, 0xfc]
        assert b[0x7b] == 57344.0 and b[0x01] == 2.0 ** -16
    assert b.view(np.uint32)[0x80] == 0x80000000 and b.view(np.uint32)[0x00] == 0


@pytest.mark.parametrize("fmt", FP8, ids=[NAMES[f] for f in FP8])
def test_every_finite_code_is_exact_in_f16_and_bf16(fmt):
    """So the gather has no rounding mode to choose, and the GPU tests may compare bitwise."""
    t = truth(fmt)
    finite = np.isfinite(t)
    codes = np.arange(256, dtype=np.uint8)
    for dt in (F16, BF16, F32):
        back = to_f32(decode_bits(codes, fmt, dt), dt)
        assert np.array_equal(back[finite].view(np.uint32), t[finite].view(np.uint32)), dt


def test_dtype_codes_and_sizes():
    from xgnn_amd import lib, ops
    h = lib()
    assert h.ggms_dtype_bytes(16) == 1 and h.ggms_dtype_bytes(17) == 1
    assert [h.ggms_dtype_bytes(c) for c in range(9, 16)] == [0] * 7
    assert [h.ggms_dtype_bytes(c) for c in (8, 18, -1, 99)] == [0, 0, 0, 0]
    assert ops.DTYPE_CODE[torch.float8_e4m3fn] == E4M3 and ops.DTYPE_CODE[torch.float8_e5m2] == E5M2


@pytest.mark.parametrize("src", ["F32", "F16"])
def test_quantize_features_round_trip(tmp_path, src):
    """E4M3 saturates at +-448 (torch's cast alone would give NaN beyond it), E5M2 overflows to inf; values that are
    FP8 numbers come back unchanged; every other file of the dataset is carried over."""
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    n, dim = 300, 6
    ip, ix = powerlaw_csr(n, mean_deg=5, seed=1)
    feat = np.random.RandomState(2).standard_normal((n, dim)).astype(np.float32) * 100
    feat[0, :4] = [1e6, -1e6, 448.0, -0.0]
    feat[1, :4] = [0.5, 3.0, -1.75, 2.0 ** -6]  # numbers of both formats
    if src == "F16":
        with np.errstate(over="ignore"):
            feat = feat.astype(np.float16)  # 1e6 -> inf
    g = dict(indptr=ip, indices=ix, train_set=np.arange(50, dtype=np.uint32), meta=dict(feat_dim=dim, num_class=3))
    d_in = datagen.write_dataset(str(tmp_path / "in"), g, feat=feat, label=np.zeros(n, np.int64), feat_dtype=src)
    for fmt in FP8:
        d_out = datagen.quantize_features(d_in, str(tmp_path / NAMES[fmt]), NAMES[fmt])
        q = np.fromfile(os.path.join(d_out, "feat.bin"), np.uint8).reshape(n, dim)
        vals = truth(fmt)[q]
        want = torch.from_numpy(feat.astype(np.float32))
        if fmt == E4M3:
            assert np.isfinite(vals).all()  # the clamp: +-1e6 (and an f16 table's +-inf) saturate
            assert vals[0, 0] == 448.0 and vals[0, 1] == -448.0 and vals[0, 2] == 448.0
            want = want.clamp(-448.0, 448.0)
        else:
            assert vals[0, 0] == np.inf and vals[0, 1] == -np.inf
        assert not np.isnan(vals).any()
        assert vals[0, 3] == 0 and np.signbit(vals[0, 3])
        assert vals[1, :4].tolist() == [0.5, 3.0, -1.75, 2.0 ** -6]
        # the table is torch's round-to-nearest-even cast of the (clamped) values
        assert np.array_equal(q, want.to(TORCH[fmt]).view(torch.uint8).numpy())
        with open(os.path.join(d_out, "meta.txt")) as f:
            meta = dict(line.split() for line in f)
        assert meta["FEAT_DATA_TYPE"] == NAMES[fmt] and meta["NUM_NODE"] == str(n) and meta["FEAT_DIM"] == str(dim)
        for name in ("indptr.bin", "indices.bin", "train_set.bin", "label.bin", "cache_by_degree.bin"):
            with open(os.path.join(d_in, name), "rb") as a, open(os.path.join(d_out, name), "rb") as b:
                assert a.read() == b.read(), name


def test_write_dataset_takes_fp8_tensors_and_bytes(tmp_path):
    from graphgen import powerlaw_csr
    from xgnn_amd import datagen
    ip, ix = powerlaw_csr(40, mean_deg=3, seed=1)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(8, dtype=np.uint32), meta=dict(feat_dim=4, num_class=3))
    b = np.arange(160, dtype=np.uint8).reshape(40, 4)
    for fmt in FP8:
        for how, feat in (("tensor", torch.from_numpy(b).view(TORCH[fmt])), ("bytes", b)):
            d = datagen.write_dataset(str(tmp_path / f"{NAMES[fmt]}{how}"), g, feat=feat, feat_dtype=NAMES[fmt])
            assert np.array_equal(np.fromfile(os.path.join(d, "feat.bin"), np.uint8), b.ravel())
            with open(os.path.join(d, "meta.txt")) as f:
                assert f"FEAT_DATA_TYPE\t{NAMES[fmt]}\n" in f.read()
    with pytest.raises(AssertionError):
        datagen.write_dataset(str(tmp_path / "bad"), g, feat=b.astype(np.float32), feat_dtype="F8E4M3")
