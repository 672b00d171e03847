"""GGMS_MXFP4 on a host without a GPU: the row size, the numpy tools of xgnn_amd/datagen.py against a float64 brute
force over the 16 values, the refusals that launch nothing, and the config key `feat_store_dtype = MXFP4`."""
import ctypes as C

import numpy as np
import pytest

import xgnn_amd
from config_run import run_config
from feat_formats import BF16, F16, F32, write_finite_dataset
from mxfp4_ref import MAGNITUDES, MXFP4, decode, stride
from xgnn_amd import datagen, ops

F32_MAX = np.float32(3.4028235e38)
ALL_ONES = 0xFFFFFFFF


def test_row_bytes():
    h = xgnn_amd.lib()
    assert [h.ggms_row_bytes(MXFP4, d) for d in (2, 32, 34, 100, 128, 768)] == [24, 24, 40, 72, 72, 408]
    assert [stride(d) for d in (2, 34, 128, 768, 1024)] == [datagen.mxfp4_stride(d) for d in (2, 34, 128, 768, 1024)] == [24, 40, 72, 408, 544]
    assert h.ggms_dtype_bytes(MXFP4) == 0 and ops.MXFP4 == MXFP4 and ops.row_bytes(MXFP4, 128) == 72


@pytest.mark.parametrize("dim", [2, 34, 100, 128])
def test_pack_unpack_round_trip(dim):
    rs = np.random.RandomState(dim)
    codes, scales = rs.randint(0, 16, (9, dim)).astype(np.uint8), rs.randint(0, 256, (9, (dim + 31) // 32)).astype(np.uint8)
    rows = datagen.pack_mxfp4(codes, scales)
    assert rows.shape == (9, stride(dim)) and (rows[0, 0] & 0xF, rows[0, 0] >> 4) == (codes[0, 0], codes[0, 1])
    assert not rows[:, 17 * scales.shape[1]:].any() and not rows[:, dim // 2:16 * scales.shape[1]].any()  # pad bytes, pad nibbles
    got = datagen.unpack_mxfp4(rows, dim)
    assert np.array_equal(got[0], codes) and np.array_equal(got[1], scales)
    ok = np.repeat(scales, 32, axis=1)[:, :dim] != 255
    assert np.array_equal(datagen.decode_mxfp4(codes, scales)[ok], decode(codes, scales)[ok])


def brute_force(v):
    """quantize_mxfp4's rule in float64, one block at a time: the nearest of the 8 magnitudes, a tie to the even code."""
    v = np.asarray(v, np.float32)
    codes, scales = np.zeros(v.shape, np.uint8), []
    for r, row in enumerate(v):
        scales.append([])
        for b in range(0, row.size, 32):
            blk = row[b:b + 32].astype(np.float64)
            amax = np.float32(np.abs(blk).max())
            x = int(np.clip((int(amax.view(np.uint32)) >> 23) - 2, 2, 252))
            for i, s in enumerate(np.abs(blk) * 2.0 ** (127 - x)):
                dist = np.abs(MAGNITUDES - s)
                best = [m for m in range(8) if dist[m] == dist.min()]
                codes[r, b + i] = [m for m in best if m % 2 == 0 or len(best) == 1][0] | (8 if np.signbit(blk[i]) else 0)
            scales[-1].append(x)
    return codes, np.array(scales, np.uint8)


def edge_rows(dim=64):
    """The seven ties (and their f32 neighbours) under amax 6, 4 and 3 x 2^k, +-0, saturation, an all-zero block, a block
    whose amax is the largest f32, an f32-subnormal block, and random rows of scales 10^[-30, 30]."""
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
    near = np.concatenate([ties, np.nextafter(ties, np.float32(9)), np.nextafter(ties, np.float32(0)), -ties, [0.0, -0.0, 6.0, 7.0, 7.99]])
    rows = [np.resize(near * np.float32(k), dim) for k in (1.0, 2.0 ** 40, 2.0 ** -100)]
    rows += [np.where(np.arange(dim) % 3 == 0, 4.0, np.resize(near, dim)), np.where(np.arange(dim) % 5 == 0, 3.0, np.resize(near, dim))]
    rows += [np.zeros(dim), np.where(np.arange(dim) < 32, 0.0, 1.0), np.where(np.arange(dim) == 3, F32_MAX, np.resize(near, dim) * 1e37),
             np.resize(np.array([1e-45, 6e-39, -1.1e-38, 2.9e-39, 0.0], np.float32), dim)]
    rs = np.random.RandomState(4)
    rows += list(rs.standard_normal((8, dim)) * 10.0 ** rs.uniform(-30, 30, (8, 1)))
    return np.array(rows).astype(np.float32)


@pytest.mark.parametrize("dim", [64, 34])
def test_quantize_against_the_brute_force(dim):
    v = edge_rows(64)[:, :dim]  # (dim 34: a partial last block, its amax over two elements)
    codes, scales = datagen.quantize_mxfp4(v)
    want_codes, want_scales = brute_force(v)
    assert np.array_equal(scales, want_scales) and np.array_equal(codes, want_codes)
    assert scales[5, 0] == 2 and scales[7, 0] == 252 and codes[0, 28:30].tolist() == [0, 8]  # all zero; f32 max; +-0
    # half of the widest step (2, between 4 and 6) or, saturated, less than 8 - 6: 2 x 2^(x - 127) either way
    err = np.abs(decode(codes, scales).astype(np.float64) - v)
    assert (err <= 2.0 ** (np.repeat(scales, 32, axis=1)[:, :dim].astype(np.float64) - 126)).all()
    with pytest.raises(ValueError, match="row 12 holds NaN or inf"):
        datagen.quantize_mxfp4(np.where(np.arange(3)[:, None] == 2, np.inf, v[:3]), first_row=10)


def test_refusals_launch_nothing():
    """Host buffers stand in for device memory: an argument error returns before any pointer is used."""
    h = xgnn_amd.lib()
    buf = np.zeros(1024, np.uint64)
    p, idx = buf.ctypes.data, buf.ctypes.data + 4096

    def gather(src_dt, dst_dt, dim, src=p):
        return h.ggms_gather_scatter_convert(C.c_void_p(p + 2048), C.c_void_p(src), C.c_void_p(idx), None, 4, None, dim, src_dt,
                                             dst_dt, ALL_ONES, None)
    assert gather(MXFP4, F32, 33) == -1 and b"even" in h.ggms_last_error()
    for pair in [(F32, MXFP4), (MXFP4, MXFP4), (MXFP4, 3), (MXFP4, 16), (18, MXFP4)]:
        assert gather(*pair, 32) == -1 and b"no conversion" in h.ggms_last_error(), pair
    assert gather(MXFP4, BF16, 32, src=p + 4) == -1 and b"8-byte aligned" in h.ggms_last_error()
    assert h.ggms_gather_scatter(C.c_void_p(p + 2048), C.c_void_p(p), C.c_void_p(idx), None, 4, None, 32, MXFP4, None) == -1

    def quantize(out, src_dt, dim):
        return h.ggms_quantize_rows(C.c_void_p(out), MXFP4, C.c_void_p(p), src_dt, 2, dim, 0, None, None)
    assert quantize(p + 2048, F32, 33) == -1 and b"even" in h.ggms_last_error()
    assert quantize(p + 2052, F16, 32) == -1 and quantize(p + 2048, BF16, 32) == -1 and quantize(p + 2048, MXFP4, 32) == -1


def test_config_takes_the_store_type_with_feat_out_dtype_only(tmp_path):
    d = write_finite_dataset(tmp_path / "f32x20", F32, 20)
    out = run_config(d["path"], dict(feat_store_dtype="MXFP4", feat_out_dtype="bf16"))
    assert out.returncode == 0 and out.stdout.split()[:1] == ["configured"], out.stderr[-2000:]
    out = run_config(d["path"], dict(feat_store_dtype="MXFP4"))
    assert out.returncode < 0 and "FEAT_DATA_TYPE MXFP4 needs the config key feat_out_dtype" in out.stderr, out.stderr[-2000:]
    q = datagen.quantize_features(d["path"], str(tmp_path / "mx"), "MXFP4", chunk_rows=1000)
    assert open(f"{q}/feat.bin", "rb").read() == datagen.pack_mxfp4(*datagen.quantize_mxfp4(d["values"])).tobytes()
    assert run_config(q, dict(feat_out_dtype="f16")).returncode == 0 and run_config(q, {}).returncode < 0
