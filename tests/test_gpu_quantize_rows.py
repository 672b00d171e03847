"""ggms_quantize_rows on the GPU (ops.quantize_rows, datagen.quantize_features(device=...)): every output byte equals
what the CPU tools compute -- the torch casts for F16 / BF16 / FP8, datagen.quantize_q8row + pack_q8row for Q8ROW.  The
expected bytes never come from the library."""
import os

import numpy as np
import pytest
import torch

from feat_formats import (BF16, CODES, F16, F32, TORCH, assert_bits, assert_fp8_bytes, cpu_q8row, from_f32, q8row_table, stride,
                          tensor_bits, write_finite_dataset)
from xgnn_amd import datagen, ops
from xgnn_amd._lib import GgmsError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG_DIM = 1024  # the longest row the register kernel takes (quantize.hip: kRegDim); 1032 takes the two-pass kernel


def _gpu_bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


# ---- FP8 / F16 / BF16 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["F8E4M3", "F8E5M2"])
def test_fp8_from_every_f16(fmt):
    half = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(512, 128)
    got = _gpu_bytes(ops.quantize_rows(torch.from_numpy(half).to(DEV), TORCH[CODES[fmt]]))
    assert_fp8_bytes(got, half.astype(np.float32), fmt, f"f16 -> {fmt}")


def _edge_table(codes):
    """codes (finite f32 values of the target, ascending and distinct), the midpoint of every neighbouring pair, each
    midpoint's two f32 neighbours, and the fixed list of the saturation / overflow / subnormal edges: (rows, 20) f32."""
    codes = np.unique(codes[np.isfinite(codes)]).astype(np.float32)
    mid = ((codes[:-1].astype(np.float64) + codes[1:].astype(np.float64)) / 2).astype(np.float32)  # exact in f32
    fixed = [448.0, 464.0, 480.0, 57344.0, 61440.0, 65504.0, 65520.0, 0.0, np.inf, 2.0 ** -10, 2.0 ** -17, 1e-45, 3.4028235e38]
    fixed = np.array(fixed + [-v for v in fixed] + [np.nan], np.float32)
    v = np.concatenate([codes, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), fixed])
    v = np.concatenate([v, np.zeros(-v.size % 20, np.float32)])
    return v.reshape(-1, 20)


def _all_codes(dt):
    if dt.itemsize == 1:
        return torch.arange(256, dtype=torch.uint8).view(dt).float().numpy()
    bits = np.random.RandomState(11).randint(0, 1 << 16, 4096).astype(np.int16)
    return torch.from_numpy(bits).view(dt).float().numpy()


@pytest.mark.parametrize("fmt", ["F8E4M3", "F8E5M2"])
def test_fp8_from_f32_codes_ties_and_edges(fmt):
    v = _edge_table(_all_codes(TORCH[CODES[fmt]]))
    got = _gpu_bytes(ops.quantize_rows(torch.from_numpy(v).to(DEV), TORCH[CODES[fmt]]))
    assert_fp8_bytes(got, v, fmt, f"f32 -> {fmt}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["F16", "BF16"])
def test_16_bit_from_f32_codes_ties_and_edges(dt):
    tdt = TORCH[dt]
    v = _edge_table(_all_codes(tdt))
    got = tensor_bits(ops.quantize_rows(torch.from_numpy(v).to(DEV), tdt), dt)
    assert_bits(got, tensor_bits(torch.from_numpy(v).to(tdt), dt), np.isnan(v), f"f32 -> {tdt}", dt=dt)


def test_bf16_from_every_f16():
    half = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(512, 128)
    got = tensor_bits(ops.quantize_rows(torch.from_numpy(half).to(DEV), torch.bfloat16), BF16)
    assert_bits(got, from_f32(half.astype(np.float32), BF16), np.isnan(half), "f16 -> bf16", dt=BF16)


def test_flat_tail_and_misaligned_bases():
    """1001 x 7 elements: no whole number of 16-byte chunks; a source 4 bytes off a 16-byte boundary takes narrower loads."""
    v = np.random.RandomState(3).standard_normal(1001 * 7 + 1).astype(np.float32) * 100
    t = torch.from_numpy(v).to(DEV)
    for off in (0, 1):
        src = t[off:off + 1001 * 7].view(1001, 7)
        got = _gpu_bytes(ops.quantize_rows(src, torch.float8_e5m2))
        assert_fp8_bytes(got, v[off:off + 1001 * 7].reshape(1001, 7), "F8E5M2", f"offset {off}")


# ---- Q8ROW ---------------------------------------------------------------------------------------------------------
def _q8row_rows(rows, dim, src, seed):
    """Random normal rows, each times its own scale 10^[-30, 30] (F16: 10^[-6, 3]), and the hand-made rows in front
    (as many as `rows` has room for)."""
    rs = np.random.RandomState(seed)
    span = (-30, 30) if src == np.float32 else (-6, 3)
    with np.errstate(over="ignore"):
        v = (rs.standard_normal((rows, dim)) * 10.0 ** rs.uniform(*span, (rows, 1))).astype(src)
    v[~np.isfinite(v)] = 1.0
    ramp = np.arange(dim) % 256
    big = 3e38 if src == np.float32 else 65504.0
    # range 1e-40: the scale, 3.9e-43, is an f32 subnormal (a range of 1e-44 gives 3.9e-47, which rounds to 0: the row
    # after it); f16 has no such range: one subnormal step, 6e-8
    tiny = 1e-40 if src == np.float32 else 6e-8
    special = [
        np.full(dim, 3.25),                                              # constant
        np.zeros(dim),                                                    # all zero
        np.where(np.arange(dim) == 0, 0.0, -0.0),                         # -0.0 and +0.0 only (minimum: -0.0)
        np.full(dim, -0.0),
        np.where(np.arange(dim) % 2, tiny, 0.0),                          # the scale is an f32 subnormal
        np.where(np.arange(dim) % 2, 1.0 + 2.0 ** -10, 1.0),             # a range of one source ulp at 1.0
        np.where(np.arange(dim) % 2, 1e-44, 0.0) if src == np.float32 else np.zeros(dim),  # f32: range 1e-44, the scale rounds to 0
        np.where(np.arange(dim) % 2, big, -big),                          # hi - lo exceeds f32 max
        ramp.astype(np.float64),                                          # lo 0, range 255 at dim >= 256, else dim - 1
        np.where(np.arange(dim) == 0, 0.0, np.where(np.arange(dim) == dim - 1, 255.0, ramp % 255 + 0.5)),  # lo 0, scale 1: k + 0.5
        np.where(np.arange(dim) == 0, 0.0, np.where(np.arange(dim) == dim - 1, 127.5, (ramp % 255) * 0.5 + 0.25)),  # scale 0.5
        np.where(np.arange(dim) == dim // 2, big / 4, rs.standard_normal(dim)),  # one huge outlier
        np.concatenate([[9.0], rs.uniform(-1, 1, max(dim - 2, 0)), [-9.0]])[:dim] if dim > 1 else np.array([9.0]),  # max first, min last
    ]
    for i, row in enumerate(special[:rows]):
        v[i] = np.asarray(row, np.float64).astype(src)
    return v


Q8_DIMS = [1, 7, 8, 20, 128, 130, REG_DIM, REG_DIM + 8]


@pytest.mark.parametrize("src", [np.float32, np.float16], ids=["F32", "F16"])
@pytest.mark.parametrize("dim", Q8_DIMS)
def test_q8row_bytes_equal_the_cpu_tool(dim, src):
    for rows in (1, 3, 257):
        v = _q8row_rows(rows, dim, src, seed=dim * 7 + rows)
        want = cpu_q8row(v)
        if rows == 257:  # what the hand-made rows are there for
            scale = np.ascontiguousarray(want[:, stride(dim) - 8:stride(dim) - 4]).view("<f4").ravel()
            assert scale[0] == 0 and scale[1] == 0 and scale[6] == 0
            assert src != np.float32 or dim == 1 or 0 < scale[4] < 2.0 ** -126  # an f32 subnormal scale
            assert np.signbit(np.ascontiguousarray(want[2, stride(dim) - 4:]).view("<f4"))[0] or dim == 1
        got = ops.quantize_rows(torch.from_numpy(v).to(DEV), ops.Q8ROW)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (rows, stride(dim))
        got = got.cpu().numpy()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"dim {dim}, {rows} rows: rows {bad[:8].tolist()} differ; row {bad[0]}: got " \
                              f"{got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
        assert (got[:, dim:stride(dim) - 8] == 0).all()  # pad bytes


def test_q8row_misaligned_source():
    rs = np.random.RandomState(5)
    v = rs.standard_normal(64 * 20 + 1).astype(np.float32)
    src = torch.from_numpy(v).to(DEV)[1:].view(64, 20)  # 4 bytes off: 4-byte loads
    assert src.data_ptr() % 16 == 4
    np.testing.assert_array_equal(ops.quantize_rows(src, ops.Q8ROW).cpu().numpy(), cpu_q8row(v[1:].reshape(64, 20)))
    h = rs.standard_normal(64 * 20 + 1).astype(np.float16)
    src = torch.from_numpy(h).to(DEV)[1:].view(64, 20)  # 2 bytes off: the source must be 4-byte aligned
    with pytest.raises(GgmsError, match="4-byte aligned"):
        ops.quantize_rows(src, ops.Q8ROW)


def test_q8row_bad_rows():
    v = np.random.RandomState(6).standard_normal((64, 20)).astype(np.float32)
    v[5, 7], v[40, 0] = np.nan, -np.inf
    t = torch.from_numpy(v).to(DEV)
    with pytest.raises(ValueError, match=r"row 1005 holds NaN or inf"):
        ops.quantize_rows(t, ops.Q8ROW, first_row=1000)
    got = ops.quantize_rows(t, ops.Q8ROW, first_row=1000, check=False).cpu().numpy()
    assert not got[5].any() and not got[40].any()
    good = np.setdiff1d(np.arange(64), [5, 40])
    np.testing.assert_array_equal(got[good], cpu_q8row(v[good]))
    assert _gpu_bytes(ops.quantize_rows(t, torch.float8_e5m2)).shape == (64, 20)  # the other formats never report


def test_q8row_round_trip_through_the_gather():
    """The gather's decode of the GPU-made table is feat_formats' decode of the CPU-made one."""
    v = _q8row_rows(300, 20, np.float32, seed=9)[13:] * np.float32(1e-3)  # (q8row_table wants scales of 0 or >= 2^-100)
    v = v[np.abs(v).max(axis=1) < 1e30]
    codes, scale, bias = datagen.quantize_q8row(v)
    keep = (scale == 0) | (scale >= 2.0 ** -100)
    v, table = v[keep], q8row_table(codes[keep], scale[keep], bias[keep])
    q = ops.quantize_rows(torch.from_numpy(np.ascontiguousarray(v)).to(DEV), ops.Q8ROW)
    out = torch.empty((v.shape[0], 20), dtype=torch.float32, device=DEV)
    ops.gather_scatter_convert(out, q, None, None, num=v.shape[0], src_dtype=ops.Q8ROW)
    np.testing.assert_array_equal(tensor_bits(out, F32), table.want(F32, np.arange(v.shape[0])))


# ---- datagen.quantize_features(device=...) -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    root = tmp_path_factory.mktemp("quantize_ds")
    return {"f32": write_finite_dataset(root / "f32x20", F32, 20), "f16": write_finite_dataset(root / "f16x128", F16, 128),
            "inf": write_finite_dataset(root / "inf_f32x20", F32, 20, bad_rows={2500: np.inf})}


@pytest.mark.parametrize("fmt", ["Q8ROW", "F8E4M3"])
@pytest.mark.parametrize("name", ["f32", "f16"])
def test_quantize_features_on_the_gpu_writes_the_cpu_files(datasets, tmp_path, name, fmt):
    d = datasets[name]
    cpu = datagen.quantize_features(d["path"], str(tmp_path / "cpu"), fmt, chunk_rows=1000)
    gpu = datagen.quantize_features(d["path"], str(tmp_path / "gpu"), fmt, chunk_rows=1000, device=DEV)
    for f in ("feat.bin", "meta.txt"):
        assert open(os.path.join(gpu, f), "rb").read() == open(os.path.join(cpu, f), "rb").read(), f
    assert sorted(os.listdir(gpu)) == sorted(os.listdir(cpu))


def test_quantize_features_on_the_gpu_16_bit_formats(datasets, tmp_path):
    out = datagen.quantize_features(datasets["f32"]["path"], str(tmp_path / "bf16"), "BF16", chunk_rows=1000, device=DEV)
    got = np.fromfile(os.path.join(out, "feat.bin"), np.uint16).reshape(3000, 20)
    np.testing.assert_array_equal(got, from_f32(datasets["f32"]["values"], BF16))
    assert open(os.path.join(out, "meta.txt")).read().endswith("FEAT_DATA_TYPE\tBF16\n")


def test_quantize_features_on_the_gpu_names_the_dataset_row(datasets, tmp_path):
    with pytest.raises(ValueError, match=r"row 2500 holds NaN or inf"):
        datagen.quantize_features(datasets["inf"]["path"], str(tmp_path / "q"), "Q8ROW", chunk_rows=1000, device=DEV)
