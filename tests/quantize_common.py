"""Shared by the feat_store_dtype / ggms_quantize_rows tests: datasets whose F32 / F16 table is finite (a row-scaled
table has no code for NaN or inf, and feat_convert_common's tables carry both on purpose), and the CPU yardsticks."""
import os

import numpy as np
import torch

from feat_convert_common import F16, F32, write_feat_dataset

NP = {F32: np.float32, F16: np.float16}
FP8 = {"F8E4M3": torch.float8_e4m3fn, "F8E5M2": torch.float8_e5m2}


def write_finite_dataset(path, dt, dim, bad_rows=()):
    """write_feat_dataset's dataset with every NaN / inf of its table replaced by 0.5 (the rounding-edge values and the
    signed zeros stay); bad_rows: {row: value} puts a non-finite value back into column 3 of those rows."""
    d = write_feat_dataset(path, dt, dim)
    v = d["feat"].view(NP[dt]).copy()
    v[~np.isfinite(v)] = 0.5
    for row, value in dict(bad_rows).items():
        v[row, 3] = value
    v.tofile(os.path.join(d["path"], "feat.bin"))
    d["values"] = v
    return d


def cpu_q8row(values, first_row=0):
    from xgnn_amd import datagen
    return datagen.pack_q8row(*datagen.quantize_q8row(values, first_row=first_row))


def cpu_fp8(values, fmt):
    """quantize_features' cast, as bytes."""
    v = torch.from_numpy(np.ascontiguousarray(values)).float()
    if fmt == "F8E4M3":
        v = v.clamp(-448.0, 448.0)
    return v.to(FP8[fmt]).view(torch.uint8).numpy()


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
